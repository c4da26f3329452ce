"""Skip-grad add + ReLU mask fused into the conv dgrad store phase.

Op level: ``conv2d_dgrad(addend=, out_mask=)`` on the glds kernel must be
BIT-IDENTICAL to the separate passes it replaces (dgrad -> add_ -> relu_bwd):
the epilogue rounds the accumulator to bf16 first, adds in fp32, rounds, then
masks.  Where the glds kernel refuses the shape, the op still honours the
contract (NT-kernel addend, relu_bwd pass) within the dgrad tolerance.

Block / model level: the ReLU-mask handshake between adjacent fused blocks
(``PDT_DGRAD_EPILOGUE``) against the gate-off sequence.  Tolerances are those
of test_gpu_models.py::test_fused_basic_block_matches_unfused (BN-stats and
wgrad atomics make two runs differ in the last bits): 3e-2 activations and
input grads, 5e-2 parameter grads.

Those absolute tolerances are wide next to gradients of 1e-3..1e-2, so runs
of the SAME composition (gate on vs gate off: the fused dgrad is bit-identical
to the passes it replaces) are also held to a bound normalised by max|ref|.
Two such runs differ only through fp32-atomics order, which surfaces as
single bf16 ulp flips (2^-8 relative) where a value is rounded; allowing 2
roundings per conv+BN layer on the way back to the input and adding them
linearly gives 16 ulps = 2^-4 for a block pair (<= 8 layers) and 40 ulps for
ResNet-18 (20 layers).  A broken handshake leaves about half of g unmasked —
errors of the order of the gradients themselves.
"""

import functools
import os

import pytest
import torch

from _errbound import conv_dgrad_ref, poison

pytestmark = pytest.mark.gpu

if torch.cuda.is_available():
    from pytorch_ddp_template_amd.ops.native import native

    EXT = native()
DEV = "cuda:0"
GATE = "PDT_DGRAD_EPILOGUE"


def _t(*shape, seed):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g)


# n, h, cin, kout, r, stride, pad -> tile / path of the glds kernel
GLDS_SHAPES = [
    (8, 8, 512, 64, 3, 1, 1),    # 256x256, 2 column tiles
    (8, 8, 128, 64, 3, 1, 1),    # 256x128
    (8, 8, 64, 64, 3, 1, 1),     # 256x64, 2 blocks/CU
    (8, 8, 192, 64, 3, 1, 1),    # 256x64, 3 column tiles
    (8, 8, 64, 128, 3, 2, 1),    # stuffed stride-2 gather
    (8, 8, 64, 128, 1, 2, 0),    # 1x1 s2 downsample dgrad, output padding 1
    (64, 14, 64, 64, 3, 1, 1),   # non-pow2 spatial (ResNet-50)
]
FALLBACK_SHAPE = (2, 8, 32, 32, 3, 1, 1)  # kout=32: glds refuses


@functools.lru_cache(maxsize=None)
def _case(n, h, cin, kout, r, stride, pad):
    """Inputs and the unfused dgrad of one shape, computed once and shared
    (callers clone before any in-place op)."""
    ho = (h + 2 * pad - r) // stride + 1
    dy = _t(n, ho, ho, kout, seed=18).to(torch.bfloat16).to(DEV)
    w = (_t(kout, r, r, cin, seed=19) * 0.1).to(torch.bfloat16).to(DEV)
    a = _t(n, h, h, cin, seed=20).to(torch.bfloat16).to(DEV)
    # a ReLU output: about half exact zeros, plus a few planted -0.0
    m = torch.relu(_t(n, h, h, cin, seed=21)).to(torch.bfloat16)
    m.view(-1)[::97] = -0.0
    assert (m.view(torch.int16) == -32768).sum() > 0
    m = m.to(DEV)
    base = EXT.conv2d_dgrad(dy, w, stride, pad, h, h)
    return dy, w, a, m, base


def _fused(shape, addend, mask):
    n, h, cin, kout, r, stride, pad = shape
    dy, w, _, _, _ = _case(*shape)
    poison(DEV, 2 * n * h * h * cin)
    return EXT.conv2d_dgrad(dy, w, stride, pad, h, h, addend=addend,
                            out_mask=mask)


def _assert_identical(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape
    same = torch.equal(got.view(torch.int16), want.view(torch.int16))
    if not same:
        # +0 / -0 and NaN payloads aside, report the value difference
        diff = (got.float() - want.float()).abs()
        bad = int((got.view(torch.int16) != want.view(torch.int16)).sum())
        raise AssertionError(
            f"{what}: {bad}/{got.numel()} elements differ bitwise, "
            f"max abs diff {diff.max().item()}")
    assert torch.equal(got, want)


@pytest.mark.parametrize("shape", GLDS_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_dgrad_addend_and_mask_bit_exact(shape):
    _, _, a, m, base = _case(*shape)
    want = EXT.relu_bwd(EXT.add_(base.clone(), a.clone()), m)
    got = _fused(shape, a, m)
    _assert_identical(got, want, "addend+out_mask")
    # masked positions really are zero, -0.0 mask entries included
    assert (got[~(m.float() > 0)] == 0).all()


@pytest.mark.parametrize("shape", GLDS_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_dgrad_addend_only_bit_exact(shape):
    _, _, a, _, base = _case(*shape)
    want = EXT.add_(base.clone(), a.clone())
    _assert_identical(_fused(shape, a, None), want, "addend")


@pytest.mark.parametrize("shape", GLDS_SHAPES, ids=lambda s: "-".join(map(str, s)))
def test_dgrad_mask_only_bit_exact(shape):
    _, _, _, m, base = _case(*shape)
    want = EXT.relu_bwd(base, m)
    _assert_identical(_fused(shape, None, m), want, "out_mask")


def test_dgrad_fallback_mask_only_exact():
    _, _, _, m, base = _case(*FALLBACK_SHAPE)
    want = EXT.relu_bwd(base, m)
    _assert_identical(_fused(FALLBACK_SHAPE, None, m), want, "fallback mask")


@pytest.mark.parametrize("with_mask", [False, True])
def test_dgrad_fallback_addend_close(with_mask):
    """The NT kernel adds before rounding, so this path is not bit-exact:
    fp32 CPU reference, the existing dgrad test's bound (0.03 of ref max)."""
    from test_gpu_ops import close_bf16

    n, h, cin, kout, r, stride, pad = FALLBACK_SHAPE
    dy, w, a, m, _ = _case(*FALLBACK_SHAPE)
    got = _fused(FALLBACK_SHAPE, a, m if with_mask else None)
    ref, _, _ = conv_dgrad_ref(dy, w, stride, pad, h, h)
    ref = ref + a.cpu().double()
    if with_mask:
        ref = torch.where(m.cpu().double() > 0, ref, torch.zeros_like(ref))
        assert (got[~(m.float() > 0)] == 0).all()
    close_bf16(got, ref, scale=ref.float().abs().max().clamp(min=0.2))


# ------------------------------------------------ block / model level -----


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


def _fwd_bwd(seq, x0):
    """One forward/backward of a block pair; returns (results, node) where
    node is the first block's autograd node (it carries the handshake)."""
    for p in seq.parameters():
        p.grad = None
    x = x0.clone().requires_grad_(True)
    mid = seq[0](x)
    out = seq[1](mid)
    out.float().square().mean().backward()
    res = {"out": out.detach().clone(), "x.grad": x.grad.clone()}
    for name, p in seq.named_parameters():
        res[name] = p.grad.clone()
    return res, mid.grad_fn


ULP = 2.0 ** -8
PAIR_ULPS, MODEL_ULPS = 16, 40  # module docstring


def _assert_close(got, ref, same_composition_ulps=None):
    assert got.keys() == ref.keys()
    for k in ref:
        tol = 3e-2 if k in ("out", "x.grad", "logits") else 5e-2
        g, r = got[k].float(), ref[k].float()
        assert torch.isfinite(g).all(), f"{k}: non-finite"
        err = (g - r).abs().max().item()
        mx = r.abs().max().item()
        print(f"DGRAD_EPI {k}: max|diff|={err:.3e} max|ref|={mx:.3e}")
        assert torch.allclose(g, r, atol=tol, rtol=tol), (
            f"{k}: max abs diff {err} (tol {tol})")
        if same_composition_ulps is not None:
            assert err <= same_composition_ulps * ULP * mx, (
                f"{k}: max abs diff {err} is {err / (ULP * mx):.1f} bf16 ulps "
                f"of max|ref|={mx} (bound {same_composition_ulps})")


def _make_pair(kind):
    from pytorch_ddp_template_amd.models.resnet import (BasicBlock, Bottleneck,
                                                        wire_blocks)

    torch.manual_seed(0)
    if kind == "basic":
        blocks = [BasicBlock(64, 64, 1), BasicBlock(64, 128, 2)]
    else:
        blocks = [Bottleneck(64, 16, 1), Bottleneck(64, 32, 2)]
    wire_blocks(blocks)
    seq = torch.nn.Sequential(*blocks).to(torch.bfloat16).to(DEV)
    seq.train()
    x0 = torch.relu(torch.randn(16, 8, 8, 64)).to(torch.bfloat16).to(DEV)
    return seq, x0


@functools.lru_cache(maxsize=None)
def _pair(kind):
    """The wired pair, its input and its gate-off results (shared)."""
    seq, x0 = _make_pair(kind)
    with _gate("0"):
        ref, node = _fwd_bwd(seq, x0)
    assert getattr(node, "dy_premasked", None) is None  # gate off: no offer
    return seq, x0, ref


@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_wired_blocks_match_gate_off(kind):
    seq, x0, ref = _pair(kind)
    with _gate("1"):
        got, node = _fwd_bwd(seq, x0)
    # the consumer accepted: the producer skipped its relu_bwd
    assert node.dy_premasked is True
    _assert_close(got, ref, PAIR_ULPS)


@pytest.mark.parametrize("kind", ["basic", "bottleneck"])
def test_consumer_fallback_keeps_producer_masking(kind):
    """Second block on the unfused module path: it does not mask its dx, so
    the producer must.  A producer that skipped its mask here gets about half
    of g wrong — far outside tolerance."""
    seq, x0, ref = _pair(kind)
    seq[1]._can_fuse = lambda _x: False
    try:
        with _gate("1"):
            got, node = _fwd_bwd(seq, x0)
        with _gate("0"):
            same, _ = _fwd_bwd(seq, x0)  # same composition, gate off
    finally:
        del seq[1]._can_fuse
    assert node.dy_premasked is False  # offered, not accepted
    _assert_close(got, ref)
    _assert_close(got, same, PAIR_ULPS)


def test_standalone_block_neither_offers_nor_accepts():
    from pytorch_ddp_template_amd.models.resnet import BasicBlock

    torch.manual_seed(0)
    blk = BasicBlock(64, 64, 1).to(torch.bfloat16).to(DEV)
    blk.train()
    x = torch.randn(16, 8, 8, 64, dtype=torch.bfloat16, device=DEV,
                    requires_grad=True)
    with _gate("1"):
        out = blk(x)
    assert out.grad_fn.dy_premasked is None and out.grad_fn.mask_in is False


def test_resnet18_matches_gate_off_under_allocator_churn():
    from pytorch_ddp_template_amd.models import resnet18
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss

    torch.manual_seed(3)
    model = resnet18(num_classes=10, stem="cifar").to(torch.bfloat16).to(DEV)
    model.train()
    crit = CrossEntropyLoss()

    def run(x, y):
        model.zero_grad(set_to_none=True)
        poison(DEV, x.numel() * 64 * 2)
        logits = model(x)
        crit(logits, y).backward()
        res = {"logits": logits.detach().clone()}
        for name, p in model.named_parameters():
            assert p.grad is not None, name
            res[name] = p.grad.clone()
        return res

    for batch in (64, 192):
        x = torch.randn(batch, 32, 32, 3).to(torch.bfloat16).to(DEV)
        y = torch.randint(0, 10, (batch,)).to(DEV)
        with _gate("0"):
            ref = run(x, y)
        with _gate("1"):
            got = run(x, y)
        _assert_close(got, ref, MODEL_ULPS)
