"""Fused window attention (ops/csrc/window_attention.hip) against the float64
reference of _winref.py, and the Swin model built on it.  The bounds are those
of fused attention in test_gpu_attn_dropout.py."""

import copy
import functools

import pytest
import torch

import _errbound as eb
import _winref as wr
from pytorch_ddp_template_amd.ops import CrossEntropyLoss, window_attention
from pytorch_ddp_template_amd.ops import functional as X
from pytorch_ddp_template_amd.ops.native import native as _ext

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SCALE = 32 ** -0.5
BOUNDS = {"out": 0.03, "dqkv": 0.05, "dbias": 0.05}

# (n, h, w, heads, shift): one window with a partial workgroup; one window that
# wraps on all sides; 2x2 windows with all 9 regions; H != W and more heads
# than waves; the unshifted path
SHAPES = [(1, 7, 7, 3, 0), (1, 7, 7, 1, 3), (2, 14, 14, 3, 3),
          (1, 14, 21, 6, 3), (2, 14, 14, 3, 0)]


@functools.lru_cache(maxsize=None)
def _case(shape, dtype):
    n, h, w, heads, shift = shape
    qkv, table, dout = wr.inputs(n, h, w, heads, dtype)
    return (qkv, table, dout), wr.win_attn_ref(qkv, table, heads, shift, SCALE,
                                               dout)


def _check(what, got, ref):
    for name, g, r in zip(BOUNDS, got, ref):
        err = eb.rel_err(g.float(), r)
        print(f"WINATTN {what} {name} rel_err={err:.5f}")
        assert err <= BOUNDS[name], f"{what} {name}: {err}"


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16],
                         ids=["bf16", "f16"])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_match_float64(shape, dtype):
    (qkv, table, dout), ref = _case(shape, dtype)
    heads, shift = shape[3], shape[4]
    qkv, table, dout = qkv.to(DEV), table.to(DEV), dout.to(DEV)
    eb.poison(DEV, qkv.numel() * 2)
    out = _ext().win_attn_fwd(qkv, table, heads, shift, SCALE)
    eb.poison(DEV, qkv.numel() * 2)
    dqkv, dbias = _ext().win_attn_bwd(dout, qkv, table.float(), heads, shift,
                                      SCALE)
    assert dbias.dtype == torch.float32 and dqkv.dtype == dtype
    _check(f"{shape} {dtype}", (out, dqkv, dbias), ref)


def test_dbias_repeatable_and_autograd_is_the_kernels():
    shape = (2, 14, 14, 3, 3)
    qkv, table, dout = (t.to(DEV) for t in _case(shape, torch.bfloat16)[0])
    out = _ext().win_attn_fwd(qkv, table, 3, 3, SCALE)
    dqkv, dbias = _ext().win_attn_bwd(dout, qkv, table, 3, 3, SCALE)
    assert torch.equal(dbias, _ext().win_attn_bwd(dout, qkv, table, 3, 3,
                                                  SCALE)[1])
    qkv.requires_grad_(True)
    table.requires_grad_(True)
    y = window_attention(qkv, table, 3, 3, SCALE)
    y.backward(dout)
    assert torch.equal(y, out) and torch.equal(qkv.grad, dqkv)
    assert table.grad.dtype == torch.bfloat16
    assert torch.equal(table.grad, dbias.to(torch.bfloat16))


def test_composed_route_on_gpu_within_the_same_bounds():
    shape = (2, 14, 14, 3, 3)
    (qkv, table, dout), ref = _case(shape, torch.bfloat16)
    qkv = qkv.to(DEV).requires_grad_(True)
    table = table.to(DEV).requires_grad_(True)
    out = X._window_attention_composed(qkv, table, 3, 3, SCALE)
    out.backward(dout.to(DEV))
    _check("composed bf16", (out, qkv.grad, table.grad), ref)


def test_errors():
    table = torch.zeros(169, 2, device=DEV)
    for h, c, shift in ((8, 192, 0), (7, 96, 0), (7, 192, 7)):
        qkv = torch.zeros(1, h, 7, c, device=DEV, dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match="win_attn_fwd"):
            _ext().win_attn_fwd(qkv, table, 2, shift, SCALE)


def _batch(seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(4, 28, 28, 3, generator=g),
            torch.randint(0, 10, (4,), generator=g))


def test_swin_bf16_close_to_cpu_f32():
    m = wr.tiny_swin()
    mg = copy.deepcopy(m).to(torch.bfloat16).to(DEV)
    x, y = _batch(6)
    ref = m(x)
    CrossEntropyLoss()(ref, y).backward()
    out = mg(x.to(torch.bfloat16).to(DEV))
    CrossEntropyLoss()(out, y.to(DEV)).backward()

    def table(mod):
        return mod.stages[0][1].attn.relative_position_bias_table.grad

    pairs = {"logits": (out, ref), "bias table": (table(mg), table(m)),
             "patch embed": (mg.patch_embed.weight.grad,
                             m.patch_embed.weight.grad)}
    for name, (got, want) in pairs.items():
        err = (got.detach().float().cpu() - want.detach()).abs().max()
        scale = want.detach().abs().max().clamp(min=1.0 if name == "logits" else 0)
        print(f"SWIN {name} err/scale={float(err / scale):.4f}")
        # the bound of test_gpu_dwconv.py test_convnext_bf16_close_to_cpu_f32
        assert err / scale < 0.12, f"{name}: relative error {err / scale}"


def test_swin_step_under_graph_capture():
    from pytorch_ddp_template_amd.optim import SGD

    m = wr.tiny_swin().to(torch.bfloat16).to(DEV)
    opt = SGD(m.parameters(), lr=0.05, momentum=0.9, master_weights=True)
    crit = CrossEntropyLoss()
    x, y = _batch(7)
    x, y = x.to(torch.bfloat16).to(DEV), y.to(DEV)
    lr_dev = torch.full((), 0.05, dtype=torch.float32, device=DEV)

    def step():
        loss = crit(m(x), y)
        loss.backward()
        opt.step(lr_tensor=lr_dev)
        m.zero_grad(set_to_none=False)
        return loss

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):  # the capture recipe of bench.py
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        loss = step()
    losses = []
    for _ in range(3):
        graph.replay()
        losses.append(float(loss))
    assert all(v == v and abs(v) < 1e4 for v in losses), losses
    assert len(set(losses)) == 3, losses
