"""ReLU-mask handshake between residual blocks: wiring and per-forward
agreement logic (no GPU needed; the numerics are in
test_gpu_dgrad_epilogue.py)."""

import torch

from pytorch_ddp_template_amd.models.resnet import (BasicBlock, Bottleneck,
                                                    resnet18, resnet50)
from pytorch_ddp_template_amd.ops import fused_block


def _blocks(model):
    return [b for layer in (model.layer1, model.layer2, model.layer3,
                            model.layer4) for b in layer]


def test_resnet_wires_consecutive_blocks():
    for model, n in ((resnet18(), 8), (resnet50(), 16)):
        blocks = _blocks(model)
        assert len(blocks) == n
        # the stem output's grad is not masked by the first block; the last
        # block keeps its own mask (the average pool does not mask)
        assert [b._in_from_block for b in blocks] == [False] + [True] * (n - 1)
        assert [b._out_to_block for b in blocks] == [True] * (n - 1) + [False]


def test_standalone_blocks_are_not_wired():
    for blk in (BasicBlock(64, 64), Bottleneck(64, 16)):
        assert blk._out_to_block is False and blk._in_from_block is False


def test_wiring_adds_no_state():
    # plain attributes only: nothing new in state_dict / submodules
    model = resnet18()
    assert not any("_block" in k for k in model.state_dict())
    assert not any("_block" in n for n, _ in model.named_modules())


class _Producer(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, offered):
        ctx.dy_premasked = False if offered else None
        return x * 2

    @staticmethod
    def backward(ctx, g):
        return g * 2, None


def _out(offered):
    x = torch.ones(3, requires_grad=True)
    return _Producer.apply(x, offered)


def test_accept_needs_offer_wiring_and_gate():
    y = _out(True)
    assert fused_block._accept_premask(y, accept=False, epi=True) is False
    assert fused_block._accept_premask(y, accept=True, epi=False) is False
    assert y.grad_fn.dy_premasked is False  # nothing agreed so far
    assert fused_block._accept_premask(y, accept=True, epi=True) is True
    assert y.grad_fn.dy_premasked is True


def test_accept_refuses_inputs_no_producer_offered():
    # producer made no offer (standalone / gate off at its forward)
    y = _out(False)
    assert fused_block._accept_premask(y, True, True) is False
    assert y.grad_fn.dy_premasked is None
    # the offered tensor went through another op first: not the same node
    z = _out(True)
    assert fused_block._accept_premask(z + 0, True, True) is False
    assert z.grad_fn.dy_premasked is False
    # a leaf (e.g. a test's randn input) has no producer at all
    leaf = torch.ones(3, requires_grad=True)
    assert fused_block._accept_premask(leaf, True, True) is False


def test_gate_env_read_at_call_time(monkeypatch):
    monkeypatch.delenv("PDT_DGRAD_EPILOGUE", raising=False)
    assert fused_block._use_dgrad_epilogue() is True
    monkeypatch.setenv("PDT_DGRAD_EPILOGUE", "0")
    assert fused_block._use_dgrad_epilogue() is False
    monkeypatch.setenv("PDT_DGRAD_EPILOGUE", "1")
    assert fused_block._use_dgrad_epilogue() is True
