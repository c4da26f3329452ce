"""Attention-probability dropout without a GPU: the mask map of ops/rng.py,
the CPU route of ``attention(..., p)`` against float64, the argument errors."""

import numpy as np
import pytest
import torch

from pytorch_ddp_template_amd.ops import rng
from pytorch_ddp_template_amd.ops.functional import attention


def _state(next_call=0, step=0):
    rng.set_state({"seed": (0x5EED << 32) | 0xC0FFEE, "rank": 3,
                   "next_call": next_call, "step": step})


def test_map_is_injective_and_the_kept_fraction_is_the_effective_rate():
    c0, j = rng.attn_draw_index(2, 65)
    assert c0.shape == j.shape == (2, 65, 65) and int(j.max()) == 15
    flat = (c0 * np.uint64(16) + j).reshape(-1)
    assert np.unique(flat).size == flat.size
    _state()
    keep = rng.attn_keep_mask(4, 197, 0.5, call_id=7, step=3)
    q = 1.0 - rng.attn_keep_threshold(0.5) / 256.0
    sigma = (q * (1.0 - q) / keep.numel()) ** 0.5
    assert abs(keep.double().mean().item() - q) <= 4.0 * sigma
    assert rng.attn_keep_scale(0.5) == float(np.float32(1.0 / q))


@pytest.mark.parametrize("p", [0.1, 0.5])
def test_cpu_attention_equals_float64_masked_softmax(p):
    B, S, d, scale = 3, 65, 16, 0.25
    g = torch.Generator().manual_seed(1)
    q, k, v = (torch.randn(B, S, d, generator=g) * 0.5 for _ in range(3))
    _state(next_call=11, step=2)
    out = attention(q, k, v, scale, p)
    keep = rng.attn_keep_mask(B, S, p, 11, 2)
    assert 0 < int(keep.sum()) < keep.numel()
    pm = torch.softmax(q.double() @ k.double().transpose(1, 2) * scale, -1)
    ref = (pm * keep * rng.attn_keep_scale(p)) @ v.double()
    # fp32 throughout: S roundings in the softmax sum, S in the PV sum and a
    # handful per element, each 2^-24 of a row's sum(P~ |v|) <= s * max|v|
    bound = (2 * S + 8) * 2.0 ** -24 * rng.attn_keep_scale(p) * v.abs().max()
    assert (out.double() - ref).abs().max() <= bound
    # eval mode and p == 0 take the plain path and no call id
    plain = attention(q, k, v, scale)
    assert torch.equal(attention(q, k, v, scale, p, training=False), plain)
    assert torch.equal(attention(q, k, v, scale, 0.0), plain)
    assert rng.get_state()["next_call"] == 12


def test_rates_that_would_drop_nothing_and_other_models_are_errors(capsys):
    from pytorch_ddp_template_amd.ddp import main
    from pytorch_ddp_template_amd.models import build_model

    q = torch.zeros(1, 4, 8)
    for bad in (1.0 / 512.0, 1.0, -0.1):
        with pytest.raises(ValueError):
            attention(q, q, q, 1.0, bad)
    assert rng.attn_keep_threshold(1.0 / 256.0) == 1
    with pytest.raises(ValueError):
        build_model("resnet18", 10, attn_dropout=0.1)
    with pytest.raises(SystemExit) as e:
        main(["--attn_dropout", "0.1", "--model", "resnet18"])
    assert e.value.code == 2
    assert "--attn_dropout" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        main(["--attn_dropout", "0.001", "--model", "vit-b16"])
    assert "1/256" in capsys.readouterr().err
