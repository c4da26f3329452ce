"""Dropout on the attention probabilities inside the fused flash kernels.
With V one-hot inside a 64-column block j, out[n, q, head, d] IS
P~[q, 64j + d]: mask and kept values are read exactly.  Oracle:
rng.attn_keep_mask; inputs randn * 0.5, scale 1/8 (every probability > 0)."""

import functools

import pytest
import torch

import _errbound as eb
from pytorch_ddp_template_amd.ops import rng
from pytorch_ddp_template_amd.ops.functional import attention, attention_qkv
from pytorch_ddp_template_amd.ops.native import native

pytestmark = pytest.mark.gpu

DEV, SCALE, N, H, DH = "cuda:0", 1.0 / 8.0, 2, 3, 64


def _state(next_call=0, step=0):
    rng.set_state({"seed": (0x5EED << 32) | 0xC0FFEE, "rank": 3,
                   "next_call": next_call, "step": step})


@functools.lru_cache(maxsize=None)
def _case(S, dtype):
    """qkv [N, S, 3, H, DH] (CPU) and the float64 softmax [N*H, S, S] of its
    q, k; shared between tests, never written to."""
    g = torch.Generator().manual_seed(S)
    qkv = (torch.randn(N, S, 3, H, DH, generator=g) * 0.5).to(dtype)
    q, k = (qkv[:, :, i].double().permute(0, 2, 1, 3).reshape(N * H, S, DH)
            for i in (0, 1))
    return qkv, torch.softmax(q @ k.transpose(1, 2) * SCALE, dim=-1)


def _ptilde(S, qkv, run):
    """[N*H, S, S] through one-hot V blocks; run(qkv) -> out [N, S, H*DH]."""
    cols = []
    for j in range((S + 63) // 64):
        x = qkv.clone()
        x[:, :, 2] = 0
        for kk in range(64 * j, min(64 * j + 64, S)):
            x[:, kk, 2, :, kk - 64 * j] = 1
        out = run(x.reshape(N, S, -1).to(DEV)).cpu()
        cols.append(out.reshape(N, S, H, DH).permute(0, 2, 1, 3)
                    .reshape(N * H, S, DH))
    return torch.cat(cols, dim=-1)[:, :, :S]


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float16])
@pytest.mark.parametrize("S", [64, 65, 197])
def test_forward_mask_is_the_oracle_and_kept_values_are_exact(S, dtype, p):
    qkv, pref = _case(S, dtype)
    cid, step = (3 << 32) | 41, 5
    _state(step=step)
    got = _ptilde(S, qkv, lambda x: native().attn_fwd(
        x, H, SCALE, False, rng.step_scalar(DEV), *rng.key(), cid, p)[0])
    keep = rng.attn_keep_mask(N * H, S, p, cid, step)
    assert torch.equal(got != 0, keep)
    assert (keep.any(-1) & (~keep).any(-1)).all(), "a row is all kept/dropped"
    ref = pref * rng.attn_keep_scale(p)
    rel = ((got.double() - ref).abs() / ref)[keep].max().item()
    assert rel <= 2 * eb.EPS_OUT[dtype] + 2.0 ** -16, rel


@pytest.mark.parametrize("p", [0.1, 0.5])
@pytest.mark.parametrize("S", [65, 197])
def test_values_and_grads_match_float64_autograd(S, p):
    qkv, _ = _case(S, torch.bfloat16)
    g = torch.randn(N, S, H * DH, generator=torch.Generator().manual_seed(9)
                    ).to(torch.bfloat16)
    _state(next_call=21, step=2)
    a = qkv.reshape(N, S, -1).to(DEV).requires_grad_(True)
    out = attention_qkv(a, H, SCALE, p)
    out.backward(g.to(DEV))
    assert rng.get_state()["next_call"] == 22
    keep = rng.attn_keep_mask(N * H, S, p, 21, 2)
    r = qkv.double().requires_grad_(True)
    q, k, v = (r[:, :, i].permute(0, 2, 1, 3).reshape(N * H, S, DH)
               for i in range(3))
    pm = torch.softmax(q @ k.transpose(1, 2) * SCALE, dim=-1)
    pm = pm * keep * rng.attn_keep_scale(p)
    ref = (pm @ v).reshape(N, H, S, DH).permute(0, 2, 1, 3).reshape(N, S, -1)
    ref.backward(g.double())
    e_out = eb.rel_err(out, ref.detach())
    e_dqkv = eb.rel_err(a.grad, r.grad.reshape(N, S, -1))
    print(f"ATTNDROP S={S} p={p} out={e_out:.3e} dqkv={e_dqkv:.3e}")
    assert e_out <= 0.03 and e_dqkv <= 0.05


def test_fused_and_composed_routes_drop_the_same_elements():
    S, p = 197, 0.5
    qkv, _ = _case(S, torch.bfloat16)

    def fused(x):
        _state(next_call=7, step=1)
        return attention_qkv(x, H, SCALE, p)

    def composed(x):
        _state(next_call=7, step=1)
        q, k, v = (t.reshape(N * H, S, DH).contiguous() for t in
                   x.reshape(N, S, 3, H, DH).permute(2, 0, 3, 1, 4))
        o = attention(q, k, v, SCALE, p)
        return o.reshape(N, H, S, DH).permute(0, 2, 1, 3).reshape(N, S, -1)

    a, b = _ptilde(S, qkv, fused), _ptilde(S, qkv, composed)
    assert torch.equal(a != 0, b != 0)
    assert torch.equal(a != 0, rng.attn_keep_mask(N * H, S, p, 7, 1))


def test_vit_tiny_f32_with_attn_dropout_matches_cpu():
    """The yardstick and runner of test_gpu_dropout.py's tiny-ViT test (8x the
    CPU path's own +-1-ulp input sensitivity), attn_dropout the only rate."""
    from pytorch_ddp_template_amd.models.vit import ViT
    from test_gpu_dropout import _fwd_bwd_f32 as run

    g = torch.Generator().manual_seed(13)
    x = torch.randn(4, 32, 32, 3, generator=g)
    y = torch.randint(0, 10, (4,), generator=g)
    torch.manual_seed(11)
    m, mg = (ViT(image_size=32, patch_size=8, dim=64, depth=2, heads=4,
                 num_classes=10, attn_dropout=0.1).train() for _ in range(2))
    mg.load_state_dict(m.state_dict())
    base = run(m, x, y)
    assert rng.get_state()["next_call"] == 2  # one mask per block
    noise = dict.fromkeys(base, 0.0)
    for seed in range(4):
        up = torch.randint(0, 2, x.shape,
                           generator=torch.Generator().manual_seed(100 + seed))
        xp = torch.nextafter(x, torch.where(up.bool(), 1.0, -1.0) * torch.inf)
        for k, t in run(m, xp, y).items():
            noise[k] = max(noise[k], eb.rel_err(t, base[k]))
    got = run(mg.to(DEV), x.to(DEV), y.to(DEV))
    bad = [k for k, t in base.items()
           if not eb.rel_err(got[k], t) <= 8 * noise[k]]
    assert not bad, bad


def test_captured_attention_draws_a_fresh_oracle_mask_on_every_replay():
    """Captured on a side stream as GraphStep does.  S = 64, V one-hot and
    dO[q, d] = [q == d]: out is P~ and dV[k, d] = P~[d, k]."""
    S, p = 64, 0.5
    qkv, _ = _case(S, torch.bfloat16)
    x = qkv.clone()
    x[:, :, 2] = torch.eye(S, dtype=x.dtype)[None, :, None, :]
    x = x.reshape(N, S, -1).to(DEV).requires_grad_(True)
    do = torch.eye(S, dtype=x.dtype)[None, :, None, :].expand(N, S, H, DH)
    do = do.reshape(N, S, -1).contiguous().to(DEV)

    def inner_step():
        rng.tick(DEV)
        out = attention_qkv(x, H, SCALE, p)
        return out, torch.autograd.grad(out, x, do)[0]

    _state(next_call=100)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            inner_step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    rng.set_state(dict(rng.get_state(), step=0))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        out, dqkv = inner_step()
    assert rng.get_state()["next_call"] == 103
    masks = []
    for k in (1, 2, 3):
        graph.replay()
        torch.cuda.synchronize()
        keep = rng.attn_keep_mask(N * H, S, p, 102, k).reshape(N, H, S, S)
        fwd = out.cpu().reshape(N, S, H, DH).permute(0, 2, 1, 3)
        dv = dqkv.cpu().reshape(N, S, 3, H, DH)[:, :, 2].permute(0, 2, 3, 1)
        assert torch.equal(fwd != 0, keep), f"replay {k}: forward mask"
        assert torch.equal(dv != 0, keep), f"replay {k}: backward mask"
        masks.append(keep)
    assert not any(torch.equal(masks[i], masks[j])
                   for i, j in ((0, 1), (1, 2), (0, 2)))


def test_rate_zero_and_eval_are_the_plain_kernels():
    qkv, _ = _case(197, torch.bfloat16)
    x = qkv.reshape(N, 197, -1).to(DEV)
    _state(next_call=5)
    want = native().attn_fwd(x, H, SCALE, False)[0]
    assert torch.equal(attention_qkv(x, H, SCALE), want)
    assert torch.equal(attention_qkv(x, H, SCALE, 0.0), want)
    assert torch.equal(attention_qkv(x, H, SCALE, 0.3, training=False), want)
    assert rng.get_state()["next_call"] == 5
    with pytest.raises(RuntimeError):
        native().attn_fwd(x, H, SCALE, True, rng.step_scalar(DEV),
                          *rng.key(), 1, 0.3)
