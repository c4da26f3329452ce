"""BN-sums hand-off between autograd nodes: wiring and the per-forward
offer / accept logic (no GPU needed; the numerics are in
test_gpu_dgrad_handoff_bnstats.py)."""

import torch

from pytorch_ddp_template_amd.models.resnet import (BasicBlock, Bottleneck,
                                                    resnet18, resnet50)
from pytorch_ddp_template_amd.ops import BatchNorm2dNHWC, fused_block
from pytorch_ddp_template_amd.ops.functional import batch_norm2d_nhwc

GATE = "PDT_DGRAD_HANDOFF_BNSTATS"


class _Producer(torch.autograd.Function):
    """A node that offers the pre-mask (or not) the way a fused block does."""

    @staticmethod
    def forward(ctx, x, offered):
        ctx.dy_premasked = False if offered else None
        t = x * 3
        fused_block._offer_bn_sums(ctx, t, t.mean(), t.std())
        return x * 2

    @staticmethod
    def backward(ctx, g):
        return g * 2, None


def _out(offered):
    x = torch.ones(3, requires_grad=True)
    return _Producer.apply(x, offered)


def test_gate_env_read_at_call_time(monkeypatch):
    monkeypatch.delenv(GATE, raising=False)
    assert fused_block._use_dgrad_handoff_bnstats() is True
    monkeypatch.setenv(GATE, "0")
    assert fused_block._use_dgrad_handoff_bnstats() is False
    monkeypatch.setenv(GATE, "1")
    assert fused_block._use_dgrad_handoff_bnstats() is True


def test_standalone_block_neither_offers_nor_accepts(monkeypatch):
    monkeypatch.setenv(GATE, "1")
    for blk in (BasicBlock(64, 64), Bottleneck(64, 16)):
        assert blk._out_to_block is False
        assert blk._in_from_block is False and blk._in_from_stem is False
    assert BatchNorm2dNHWC(8, act="relu")._out_to_block is False
    # no pre-mask offered -> no BN offered, no slot
    y = _out(False)
    assert not hasattr(y.grad_fn, "bn_offer")
    assert not hasattr(y.grad_fn, "bn_ws")
    # a block that did not agree to mask never accepts, whatever is offered
    z = _out(True)
    assert fused_block._accept_bn_sums(z, mask_in=False) is None
    # a leaf has no producer
    leaf = torch.ones(3, requires_grad=True)
    assert fused_block._accept_bn_sums(leaf, mask_in=True) is None


def test_only_the_cifar_stem_is_wired():
    m = resnet18(stem="cifar")
    assert m.stem[0][1]._out_to_block is True
    assert m.layer1[0]._in_from_stem is True
    # the block-to-block wiring is as before
    assert m.layer1[0]._in_from_block is False
    assert m.layer1[1]._in_from_stem is False
    for m in (resnet50(), resnet18(stem="imagenet")):
        # the maxpool sits between the stem's BN+ReLU and layer1
        assert m.stem[0][1]._out_to_block is False
        assert all(b._in_from_stem is False for layer in
                   (m.layer1, m.layer2, m.layer3, m.layer4) for b in layer)
    # plain attributes: nothing new in state_dict
    assert not any("_stem" in k or "_block" in k
                   for k in resnet18().state_dict())


def test_gate_off_leaves_no_workspace_slot(monkeypatch):
    monkeypatch.setenv(GATE, "0")
    y = _out(True)
    assert y.grad_fn.dy_premasked is False  # the mask offer is its own gate
    assert not hasattr(y.grad_fn, "bn_offer")
    assert not hasattr(y.grad_fn, "bn_ws")
    assert fused_block._accept_bn_sums(y, mask_in=True) is None
    monkeypatch.setenv(GATE, "1")
    y = _out(True)
    assert y.grad_fn.bn_ws is None and len(y.grad_fn.bn_offer) == 3
    assert fused_block._accept_bn_sums(y, mask_in=True) is y.grad_fn
    # offered under gate on, consumer's forward under gate off: not accepted
    monkeypatch.setenv(GATE, "0")
    assert fused_block._accept_bn_sums(y, mask_in=True) is None


def test_bn_relu_node_makes_no_offer_off_the_native_path(monkeypatch):
    monkeypatch.setenv(GATE, "1")
    x = torch.randn(2, 4, 4, 8, requires_grad=True)
    g, b = torch.ones(8, requires_grad=True), torch.zeros(8, requires_grad=True)
    y = batch_norm2d_nhwc(x, g, b, None, None, True, 0.1, 1e-5, "relu",
                          offer=True)
    assert y.grad_fn.dy_premasked is None
    assert not hasattr(y.grad_fn, "bn_ws")
    y.sum().backward()  # the CPU reference backward is untouched
    assert x.grad is not None and torch.isfinite(x.grad).all()


class _FakeExt:
    def __init__(self, ws):
        self.ws, self.calls = ws, []

    def conv2d_dgrad_bnstats(self, dy, w, stride, pad, H, W, mask, t, mean,
                             rstd, addend=None):
        self.calls.append(("bnstats", t, mean, rstd, addend, mask))
        return "dx", self.ws

    def conv2d_dgrad(self, dy, w, stride, pad, H, W, addend=None,
                     out_mask=None):
        self.calls.append(("dgrad", addend, out_mask))
        return "dx"


class _Ctx:
    epi, mask_in = True, True


def test_consumer_hands_the_workspace_to_the_producer(monkeypatch):
    monkeypatch.setenv(GATE, "1")
    y = _out(True)
    prod = y.grad_fn
    ctx = _Ctx()
    ctx.bn_up = fused_block._accept_bn_sums(y, mask_in=True)
    for ws in ("ws", None):  # None: the kernel declined the shape
        ext = _FakeExt(ws)
        dx = fused_block._skip_grad_dgrad(ext, ctx, "dy", "w", 1, 1, 8, 8,
                                          "addend", "x")
        assert dx == "dx" and prod.bn_ws is ws
        kind, t, mean, rstd, addend, mask = ext.calls[0]
        assert kind == "bnstats" and (addend, mask) == ("addend", "x")
        assert (t, mean, rstd) == prod.bn_offer
    # the producer's backward takes the sums and releases the offer; a second
    # backward through the consumer then runs the plain masked dgrad
    prod.bn_ws = "ws"
    assert fused_block._take_bn_ws(prod) == "ws"
    assert prod.bn_ws is None and prod.bn_offer is None
    ext = _FakeExt("ws")
    fused_block._skip_grad_dgrad(ext, ctx, "dy", "w", 1, 1, 8, 8, "addend",
                                 "x")
    assert ext.calls == [("dgrad", "addend", "x")]
    # a node that never offered has nothing to take
    assert fused_block._take_bn_ws(_out(False).grad_fn) is None
    ctx.bn_up = None
    fused_block._skip_grad_dgrad(ext, ctx, "dy", "w", 1, 1, 8, 8, "addend",
                                 "x")
    assert ext.calls[-1] == ("dgrad", "addend", "x")
