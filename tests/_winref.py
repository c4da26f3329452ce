"""Float64 reference of Swin's window attention, written from the published
formulas (roll, partition, img_mask slices, relative_position_index gather,
softmax, reverse), and the tiny model the window-attention tests share."""

import torch

WS = 7


def win_attn_ref(qkv, table, heads, shift, scale, dout):
    """(out, dqkv, dtable) in float64 for qkv [N,H,W,3*heads*dh]."""
    qkv = qkv.detach().cpu().double().requires_grad_(True)
    table = table.detach().cpu().double().requires_grad_(True)
    N, H, W, C3 = qkv.shape
    C, nW = C3 // 3, (H // WS) * (W // WS)
    x = torch.roll(qkv, (-shift, -shift), (1, 2))
    x = x.view(N, H // WS, WS, W // WS, WS, C3).permute(0, 1, 3, 2, 4, 5)
    x = x.reshape(-1, WS * WS, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = x[0] * scale, x[1], x[2]
    coords = torch.stack(torch.meshgrid(
        torch.arange(WS), torch.arange(WS), indexing="ij")).flatten(1)
    rel = coords[:, :, None] - coords[:, None, :]
    index = (rel[0] + WS - 1) * (2 * WS - 1) + rel[1] + WS - 1
    bias = table[index.view(-1)].view(WS * WS, WS * WS, heads).permute(2, 0, 1)
    attn = q @ k.transpose(-2, -1) + bias
    if shift > 0:
        img_mask = torch.zeros(1, H, W, 1, dtype=torch.float64)
        slices = (slice(0, -WS), slice(-WS, -shift), slice(-shift, None))
        for cnt, (hs, ws) in enumerate((a, b) for a in slices for b in slices):
            img_mask[:, hs, ws, :] = cnt
        mw = img_mask.view(1, H // WS, WS, W // WS, WS, 1)
        mw = mw.permute(0, 1, 3, 2, 4, 5).reshape(-1, WS * WS)
        am = mw[:, None, :] - mw[:, :, None]
        am = torch.where(am != 0, -100.0, 0.0)
        attn = attn.view(N, nW, heads, 49, 49) + am[None, :, None]
        attn = attn.view(-1, heads, 49, 49)
    o = (attn.softmax(-1) @ v).transpose(1, 2).reshape(-1, WS, WS, C)
    o = o.view(N, H // WS, W // WS, WS, WS, C).permute(0, 1, 3, 2, 4, 5)
    out = torch.roll(o.reshape(N, H, W, C), (shift, shift), (1, 2))
    out.backward(dout.detach().cpu().double())
    return out.detach(), qkv.grad, table.grad


def inputs(n, h, w, heads, dtype=torch.float32, dh=32):
    from _errbound import randn

    return (randn(n, h, w, 3 * heads * dh, seed=1, dtype=dtype),
            randn(169, heads, seed=2, dtype=dtype),
            randn(n, h, w, heads * dh, seed=3, dtype=dtype))


def tiny_swin(drop_path=0.0):
    from pytorch_ddp_template_amd.models.swin import SwinTransformer

    torch.manual_seed(5)
    return SwinTransformer(28, 2, (32, 64), (2, 2), (1, 2), num_classes=10,
                           drop_path=drop_path)
