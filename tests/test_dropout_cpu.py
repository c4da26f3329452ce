"""Philox dropout / stochastic depth on the CPU path: the generator against
the published vectors and an independent numpy oracle, the autograd rules,
the rng state (round trip, checkpoint, bit-exact resume) and the ViT / CLI
wiring.  No GPU needed."""

import argparse
import copy
import json
import math
import os

import numpy as np
import pytest
import torch

from pytorch_ddp_template_amd.ops import (
    Dropout,
    DropPath,
    drop_path,
    dropout,
    dropout_add,
    rng,
)

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")

# ------------------------------------------------ independent numpy oracle --


def philox(ctr, key):
    """Philox4x32-10.  ctr: four words (ints or uint64 arrays), key: two."""
    m = np.uint64(0xFFFFFFFF)
    c = [np.asarray(v, dtype=np.uint64) & m for v in ctr]
    k = [int(key[0]), int(key[1])]
    for _ in range(10):
        p0 = np.uint64(0xD2511F53) * c[0]
        p1 = np.uint64(0xCD9E8D57) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k[0]), p1 & m,
             (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k[1]), p0 & m]
        k = [(k[0] + 0x9E3779B9) & 0xFFFFFFFF, (k[1] + 0xBB67AE85) & 0xFFFFFFFF]
    return c


def oracle_words(n, seed, rank, call_id, step):
    """Word of element e = word (e & 3) of block (e >> 2, call lo, call hi,
    step) under key (seed lo, seed hi ^ rank)."""
    blk = np.arange((n + 3) // 4, dtype=np.uint64)
    key = (seed & 0xFFFFFFFF, ((seed >> 32) ^ rank) & 0xFFFFFFFF)
    w = philox((blk, call_id & 0xFFFFFFFF, call_id >> 32, step), key)
    return np.stack(w, axis=1).reshape(-1)[:n]


def oracle_keep(n, p, seed, rank, call_id, step):
    return oracle_words(n, seed, rank, call_id, step) >= np.uint64(
        math.floor(p * 2 ** 32))


def _state(seed=1234, rank=0, next_call=0, step=0):
    rng.set_state({"seed": seed, "rank": rank, "next_call": next_call,
                   "step": step})


def _nonzero(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=g)
    return torch.where(x == 0, torch.ones_like(x), x)


def _hex(words):
    return " ".join("%08x" % int(np.asarray(w).reshape(-1)[0]) for w in words)


# ------------------------------------------------------------ generator -----

VECTORS = [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2,
     "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344),
     (0xA4093822, 0x299F31D0), "d16cfe09 94fdcceb 5001e420 24126ea1"),
]


@pytest.mark.parametrize("ctr,key,want", VECTORS)
def test_oracle_and_host_philox_match_published_vectors(ctr, key, want):
    assert _hex(philox(ctr, key)) == want
    assert _hex(rng.philox4x32_10(*ctr, *key)) == want


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
@pytest.mark.parametrize("n", [1, 3, 4099])
def test_cpu_mask_equals_oracle(p, n):
    _state(next_call=7, step=5)
    x = _nonzero(n, seed=n)
    y = dropout(x, p, True)
    keep = oracle_keep(n, p, 1234, 0, 7, 5)
    assert np.array_equal((y != 0).numpy(), keep)
    s = np.float32(1.0 / (1.0 - p))
    want = torch.from_numpy(np.where(keep, x.numpy() * s, np.float32(0)))
    assert torch.equal(y, want)


def test_row_mask_equals_oracle_and_known_counts():
    x = _nonzero(64, 5, 3, seed=1)
    for p, kept in ((0.25, 49), (0.5, 37)):
        keep = oracle_keep(64, p, 1234, 0, 2, 0)
        assert int(keep.sum()) == kept
        _state(next_call=2)
        y = drop_path(x, p, True)
        rows = (y != 0).reshape(64, -1)
        assert np.array_equal(rows.all(1).numpy(), keep)
        assert np.array_equal(rows.any(1).numpy(), keep)
        s = np.float32(1.0 / (1.0 - p))
        assert torch.equal(y[keep], x[keep] * float(s))


@pytest.mark.parametrize("p", [0.1, 0.5, 0.9])
def test_keep_fraction(p):
    n = 1 << 20
    _state(next_call=1)
    y = dropout(torch.ones(n), p, True)
    kept = int((y != 0).sum())
    thr = math.floor(p * 2 ** 32)
    dev = abs(kept / n - (1 - thr / 2 ** 32))
    sigma = math.sqrt(p * (1 - p) / n)
    print(f"KEEPFRAC p={p} dev={dev / sigma:.2f} sigma")
    assert dev <= 4 * sigma


@pytest.mark.parametrize("change", ["seed", "rank", "next_call", "step"])
def test_changing_one_input_changes_the_mask(change):
    base = {"seed": 1234, "rank": 0, "next_call": 1, "step": 0}
    x = torch.ones(4096)
    rng.set_state(base)
    a = dropout(x, 0.5, True) != 0
    other = dict(base)
    other[change] += 1 if change != "seed" else (1 << 32)
    rng.set_state(other)
    b = dropout(x, 0.5, True) != 0
    agree = float((a == b).float().mean())
    assert 0.4 < agree < 0.6, agree
    # the low seed word alone changes it too
    rng.set_state(dict(base, seed=1235))
    c = dropout(x, 0.5, True) != 0
    assert 0.4 < float((a == c).float().mean()) < 0.6


def test_backward_is_mask_times_scale_and_residual_grad_is_dy():
    _state(next_call=3)
    x = _nonzero(6, 10, seed=2).requires_grad_(True)
    res = _nonzero(6, 10, seed=3).requires_grad_(True)
    dy = _nonzero(6, 10, seed=4)
    y = dropout_add(x, res, 0.5, 0.25, True)
    y.backward(dy)
    ke = oracle_keep(60, 0.5, 1234, 0, 3, 0).reshape(6, 10)
    kr = oracle_keep(6, 0.25, 1234, 0, 4, 0)[:, None]
    keep = torch.from_numpy(ke & kr)
    se, sr = np.float32(2.0), np.float32(1.0 / 0.75)
    want = torch.where(keep, dy * float(se) * float(sr), torch.zeros(()))
    assert torch.equal(x.grad, want)
    assert torch.equal(res.grad, dy)
    want_y = res.detach() + torch.where(
        keep, x.detach() * float(se) * float(sr), torch.zeros(()))
    assert torch.equal(y.detach(), want_y)
    assert torch.equal(y.detach()[~keep], res.detach()[~keep])


def test_eval_mode_and_zero_rate_are_identity_and_take_no_call_id():
    _state(next_call=11, step=2)
    before = rng.get_state()
    x, res = _nonzero(5, 7, seed=5), _nonzero(5, 7, seed=6)
    assert dropout(x, 0.5, False) is x
    assert dropout(x, 0.0, True) is x
    assert drop_path(x, 0.5, False) is x
    assert drop_path(x, 0.0, True) is x
    assert torch.equal(dropout_add(x, res, 0.5, 0.5, False), res + x)
    assert torch.equal(dropout_add(x, res, 0.0, 0.0, True), res + x)
    d, dp = Dropout(0.5).eval(), DropPath(0.5).eval()
    assert d(x) is x and dp(x) is x
    assert rng.get_state() == before
    assert (Dropout(0.5).train()(x) == 0).any()
    assert rng.get_state()["next_call"] == 12


def test_manual_seed_key_and_reset():
    _state(next_call=9, step=4)
    rng.manual_seed((0xABCD << 32) | 0x1234, rank=5)
    assert rng.key() == (0x1234, 0xABCD ^ 5)
    assert rng.get_state() == {"seed": (0xABCD << 32) | 0x1234, "rank": 5,
                               "next_call": 0, "step": 0}


def test_state_round_trip_and_tick():
    rng.manual_seed(77, 3)
    x = torch.ones(257)
    dropout(x, 0.5, True)
    rng.tick()
    rng.tick()
    st = rng.get_state()
    assert st == {"seed": 77, "rank": 3, "next_call": 1, "step": 2}
    a = dropout(x, 0.5, True)
    rng.manual_seed(1, 0)
    rng.set_state(st)
    assert rng.get_state() == st
    b = dropout(x, 0.5, True)
    assert torch.equal(a, b)
    assert np.array_equal((a != 0).numpy(), oracle_keep(257, 0.5, 77, 3, 1, 2))


def _ckpt_args(tmp_path):
    return argparse.Namespace(output_dir=str(tmp_path), n_gpu=0, seed=1)


def _tiny_vit(dropout_rate=0.1, drop_path_rate=0.1):
    from pytorch_ddp_template_amd.models.vit import ViT

    return ViT(image_size=32, patch_size=8, dim=64, depth=2, heads=4,
               num_classes=10, dropout=dropout_rate, drop_path=drop_path_rate)


def test_checkpoint_carries_rng_state_and_old_checkpoint_loads(tmp_path):
    import logging

    from pytorch_ddp_template_amd import ddp
    from pytorch_ddp_template_amd.optim import (
        SGD, get_linear_schedule_with_warmup)

    if ddp.logger is None:
        ddp.logger = logging.getLogger("test_dropout_cpu")
    args = _ckpt_args(tmp_path)
    model = torch.nn.Linear(2, 2)
    opt = SGD(model.parameters(), lr=0.1)
    sched = get_linear_schedule_with_warmup(opt, 1, 10)
    _state(seed=99, rank=2, next_call=41, step=6)
    want = rng.get_state()
    ddp.save_checkpoint(args, model, opt, sched, 5, epoch=1, batches_in_epoch=3)
    path = os.path.join(str(tmp_path), "checkpoint-5")
    rng.manual_seed(0, 0)
    assert ddp.load_training_state(args, path) == (1, 3)
    assert rng.get_state() == want
    # a checkpoint from before the entry existed loads as before and leaves
    # the generator alone
    f = os.path.join(path, "training_state.pt")
    st = torch.load(f, weights_only=False)
    del st["rng"]["philox"]
    torch.save(st, f)
    rng.manual_seed(5, 1)
    mine = rng.get_state()
    assert ddp.load_training_state(args, path) == (1, 3)
    assert rng.get_state() == mine


def test_resume_is_bit_exact():
    """4 steps == 2 steps, save model + optimizer + rng into fresh objects,
    2 more steps."""
    from pytorch_ddp_template_amd.ops import CrossEntropyLoss
    from pytorch_ddp_template_amd.optim import AdamW

    g = torch.Generator().manual_seed(21)
    xs = [torch.randn(4, 32, 32, 3, generator=g) for _ in range(4)]
    ys = [torch.randint(0, 10, (4,), generator=g) for _ in range(4)]
    torch.manual_seed(20)
    init = _tiny_vit().state_dict()
    crit = CrossEntropyLoss()

    def fresh():
        m = _tiny_vit()
        m.load_state_dict(init)
        m.train()
        return m, AdamW(m.parameters(), lr=1e-2, weight_decay=0.05)

    def steps(m, opt, idx):
        for i in idx:
            opt.zero_grad()
            crit(m(xs[i]), ys[i]).backward()
            opt.step()

    rng.manual_seed(7, 0)
    m, opt = fresh()
    steps(m, opt, range(4))
    want = copy.deepcopy(m.state_dict())

    rng.manual_seed(7, 0)
    m, opt = fresh()
    steps(m, opt, range(2))
    saved = copy.deepcopy((m.state_dict(), opt.state_dict(), rng.get_state()))
    assert saved[2]["next_call"] > 0
    rng.manual_seed(123, 9)  # a fresh process starts from something else
    m2, opt2 = fresh()
    m2.load_state_dict(saved[0])
    opt2.load_state_dict(saved[1])
    rng.set_state(saved[2])
    steps(m2, opt2, range(2, 4))
    got = m2.state_dict()
    assert any(not torch.equal(init[k], want[k]) for k in want)
    for k in want:
        assert torch.equal(got[k], want[k]), k


def test_vit_state_dict_keys_do_not_depend_on_the_rates():
    from pytorch_ddp_template_amd.models import build_model, vit_b16

    assert list(_tiny_vit(0.0, 0.0).state_dict()) == list(
        _tiny_vit(0.1, 0.2).state_dict())
    with open(os.path.join(GOLDEN, "vit_b16_state_dict_keys.json")) as f:
        parent_keys = json.load(f)
    assert list(vit_b16().state_dict()) == parent_keys
    m = build_model("vit-b16", 10, 0.1, 0.2)
    assert list(m.state_dict()) == parent_keys
    assert [b.p_path for b in m.blocks] == [0.2 * i / 11 for i in range(12)]
    assert all(b.p == 0.1 for b in m.blocks) and m.p == 0.1


def test_vit_rate_zero_and_eval_forward_unchanged():
    """Rates 0 (train) and rates > 0 (eval) give the bits of the
    unregularised forward and take no call id."""
    torch.manual_seed(3)
    plain = _tiny_vit(0.0, 0.0)
    reg = _tiny_vit(0.3, 0.3)
    reg.load_state_dict(plain.state_dict())
    x = torch.randn(2, 32, 32, 3)
    _state(next_call=4)
    want = plain.train()(x)
    assert torch.equal(reg.eval()(x), want)
    assert rng.get_state()["next_call"] == 4
    assert not torch.equal(reg.train()(x), want)
    assert rng.get_state()["next_call"] > 4


def test_build_model_and_cli_reject_rates_on_other_models(capsys):
    from pytorch_ddp_template_amd.ddp import main
    from pytorch_ddp_template_amd.models import build_model

    with pytest.raises(ValueError):
        build_model("resnet18", 10, 0.1, 0.0)
    with pytest.raises(SystemExit) as e:
        main(["--dropout", "0.1", "--model", "resnet18"])
    assert e.value.code == 2
    with pytest.raises(SystemExit):
        main(["--drop_path", "0.1", "--model", "foo"])
    assert "--dropout" in capsys.readouterr().err
