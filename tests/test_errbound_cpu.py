"""The oracle in _errbound.py must pass a correct fp32 result and reject a
subtly wrong one.  Runs on the CPU: the "kernel" is torch's own fp32 op, the
mutations are the mistakes a HIP kernel makes (a dropped reduction tail, a
dropped 8-element staging group, truncation instead of round-to-nearest,
tf32-like input rounding, an H/W swap in the gather decode, an unwritten
output row, a missing or doubled bias)."""

import pytest
import torch
import torch.nn.functional as F

import _errbound as eb

BF16 = torch.bfloat16


def _truncate_bf16(t):
    """fp32 -> bf16 by chopping the low 16 bits (round toward zero)."""
    bits = t.contiguous().view(torch.int32) & ~0xFFFF
    return bits.view(torch.float32).to(BF16)  # exact: low bits already zero


def _round_mantissa(t, bits=10):
    """Round fp32 to `bits` explicit mantissa bits (tf32-like), RNE-ish."""
    drop = 23 - bits
    i = t.contiguous().view(torch.int32)
    i = (i + (1 << (drop - 1))) & ~((1 << drop) - 1)
    return i.view(torch.float32)


def _conv32(x, w, b, stride, pad):
    y = F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride, pad)
    return y.permute(0, 2, 3, 1).contiguous()


def _wgrad32(dy, x, stride, pad, r):
    dw = torch.nn.grad.conv2d_weight(
        x.permute(0, 3, 1, 2), (dy.shape[3], x.shape[3], r, r),
        dy.permute(0, 3, 1, 2), stride, pad)
    return dw.permute(0, 2, 3, 1).contiguous()


# ---- the three ops: inputs, float64 oracle, fp32 "kernel" ----

M, N, K = 48, 40, 96          # NT GEMM, K <= 128
CN, CH, CW, CC, CK = 2, 6, 10, 16, 24   # non-square conv, 3x3 s1 p1


class Gemm:
    a = eb.randn(M, K, seed=1)
    b = eb.randn(N, K, seed=2)
    bias = eb.randn(N, seed=3)
    ref, mag, depth = eb.linear_ref(a, b, bias)

    @staticmethod
    def run(a=None, b=None, bias=None, nbias=1):
        a = Gemm.a if a is None else a
        b = Gemm.b if b is None else b
        return a @ b.t() + nbias * Gemm.bias


class Conv:
    x = eb.randn(CN, CH, CW, CC, seed=4)
    w = eb.randn(CK, 3, 3, CC, seed=5, scale=0.1)
    bias = eb.randn(CK, seed=6)
    ref, mag, depth = eb.conv_fwd_ref(x, w, bias, 1, 1)

    @staticmethod
    def run(x=None, w=None, nbias=1):
        x = Conv.x if x is None else x
        w = Conv.w if w is None else w
        return _conv32(x, w, nbias * Conv.bias, 1, 1)


class Wgrad:
    x = eb.randn(CN, CH, CW, CC, seed=7)
    dy = eb.randn(CN, CH, CW, CK, seed=8, scale=0.1)
    ref, mag, depth = eb.conv_wgrad_ref(dy, x, 1, 1, 3, 3)

    @staticmethod
    def run(dy=None, x=None):
        dy = Wgrad.dy if dy is None else dy
        x = Wgrad.x if x is None else x
        return _wgrad32(dy, x, 1, 1, 3)


OPS = {"gemm": Gemm, "conv": Conv, "wgrad": Wgrad}


def _zeroed(t, index):
    t = t.clone()
    t[index] = 0
    return t


def _mutant(op, mut):
    """fp32 result of `op` computed with mistake `mut` (None: not applicable)."""
    if mut == "drop_last_k":
        if op == "gemm":
            return Gemm.run(a=_zeroed(Gemm.a, (slice(None), -1)))
        if op == "conv":
            return Conv.run(w=_zeroed(Conv.w, (slice(None), -1, -1, -1)))
        return Wgrad.run(dy=_zeroed(Wgrad.dy, (-1, -1, -1)))
    if mut == "drop_last_group8":
        if op == "gemm":
            return Gemm.run(a=_zeroed(Gemm.a, (slice(None), slice(-8, None))))
        if op == "conv":
            return Conv.run(
                w=_zeroed(Conv.w, (slice(None), -1, -1, slice(-8, None))))
        return Wgrad.run(dy=_zeroed(Wgrad.dy, (-1, -1, slice(-8, None))))
    if mut == "tf32_inputs":
        if op == "gemm":
            return Gemm.run(a=_round_mantissa(Gemm.a), b=_round_mantissa(Gemm.b))
        if op == "conv":
            return Conv.run(x=_round_mantissa(Conv.x), w=_round_mantissa(Conv.w))
        return Wgrad.run(dy=_round_mantissa(Wgrad.dy), x=_round_mantissa(Wgrad.x))
    if mut == "swap_hw":
        # the gather decodes the same buffer as [N, W, H, C]
        if op == "gemm":
            return None
        if op == "conv":
            y = Conv.run(x=Conv.x.reshape(CN, CW, CH, CC))
            return y.reshape(CN, CH, CW, CK)
        return Wgrad.run(dy=Wgrad.dy.reshape(CN, CW, CH, CK),
                         x=Wgrad.x.reshape(CN, CW, CH, CC))
    if mut == "zero_row":
        out = OPS[op].run().clone()
        out.reshape(-1, out.shape[-1])[out.numel() // out.shape[-1] // 2] = 0
        return out
    if mut == "no_bias":
        return None if op == "wgrad" else OPS[op].run(nbias=0)
    if mut == "bias_twice":
        return None if op == "wgrad" else OPS[op].run(nbias=2)
    raise KeyError(mut)


MUTATIONS = ["drop_last_k", "drop_last_group8", "tf32_inputs", "swap_hw",
             "zero_row", "no_bias", "bias_twice"]


@pytest.mark.parametrize("op", list(OPS))
def test_correct_fp32_result_passes(op):
    o = OPS[op]
    used = eb.assert_gemm_close(o.run(), o.ref, o.mag, o.depth, op)
    assert used < 0.5, "torch fp32 should sit well inside the bound"


def test_correct_bf16_rounded_gemm_passes():
    out = Gemm.run().to(BF16)  # round-to-nearest-even
    eb.assert_gemm_close(out, Gemm.ref, Gemm.mag, Gemm.depth, "gemm->bf16")


@pytest.mark.parametrize("op", ["gemm", "conv"])
def test_truncated_bf16_output_fails(op):
    o = OPS[op]
    good = o.run().to(BF16)
    bad = _truncate_bf16(o.run())
    assert not eb.gemm_violations(good, o.ref, o.mag, o.depth).any()
    frac = eb.gemm_violations(bad, o.ref, o.mag, o.depth).float().mean()
    assert frac > 0.05, f"truncation caught on only {float(frac):.1%}"


NOT_APPLICABLE = {("gemm", "swap_hw"), ("wgrad", "no_bias"),
                  ("wgrad", "bias_twice")}


@pytest.mark.parametrize(
    "op,mut", [(o, m) for o in OPS for m in MUTATIONS
               if (o, m) not in NOT_APPLICABLE])
def test_mutation_fails(op, mut):
    out = _mutant(op, mut)
    o = OPS[op]
    assert eb.gemm_violations(out, o.ref, o.mag, o.depth).any(), (
        f"{op}/{mut}: the oracle accepted a wrong result")
    with pytest.raises(AssertionError):
        eb.assert_gemm_close(out, o.ref, o.mag, o.depth, f"{op}/{mut}")


def test_nonfinite_output_fails():
    out = Gemm.run().clone()
    out[3, 5] = float("nan")
    assert eb.gemm_violations(out, Gemm.ref, Gemm.mag, Gemm.depth).sum() == 1


def test_calibrated_check_floor_and_factor():
    ref = {"y": torch.linspace(-1, 1, 64, dtype=torch.float64)}
    cpu = {"y": ref["y"].float()}                     # ~fp32-exact
    ok = {"y": (ref["y"] * (1 + 2.0 ** -21)).float()}  # under the 2^-20 floor
    eb.assert_calibrated("toy", ok, cpu, ref)
    bad = {"y": (ref["y"] * (1 + 2.0 ** -16)).float()}
    with pytest.raises(AssertionError):
        eb.assert_calibrated("toy", bad, cpu, ref)
