"""Shared numerics oracle: float64 references and DERIVED tolerances.

GEMM-shaped ops (linear, bmm, conv fwd / dgrad / wgrad) are checked per
element, no element exempted, against the standard dot-product bound

    |out - ref| <= eps_out*|ref| + 1.01*(depth + 2)*2^-23*mag + 1e-30

* ``ref``  the same operation in float64 on the exact inputs the kernel sees
  (bf16/fp16 inputs are cast first, then ``.double()``).
* ``mag``  the same operation on ``|inputs|`` in float64, plus ``|bias|``.
* ``depth`` the reduction length (K; R*S*Cin; R*S*Kout for dgrad; N*HO*WO
  for wgrad).
* ``eps_out`` the unit roundoff of the OUTPUT format: 2^-8 bf16, 2^-11 fp16,
  0 for f32 (the 16-bit wgrads return f32).

2^-23 rather than 2^-24 per accumulation step leaves room for non-IEEE
intermediate rounding inside MFMA.  ReLU is 1-Lipschitz so the bound survives
a fused ReLU epilogue (``ref`` is then the post-ReLU reference and ``mag`` the
pre-ReLU magnitude).  tests/test_errbound_cpu.py proves that the bound passes
correctly-rounded results and rejects subtly wrong ones.

Non-GEMM fp32 ops (norms, softmax, losses, pools, gelu, col_sum) have no
clean bound; ``assert_calibrated`` calibrates at test time against the
project's own CPU fp32 branch:  err_gpu <= max(16*err_cpu, 2^-20), errors
being max-abs vs float64 normalised by max|ref|.  16 = 4x for hardware
rsqrt/exp/divide approximations x 4x for a different association order; the
floor is 8 fp32 ulps for the case where the CPU result happens to be exact.
"""

import torch
import torch.nn.functional as F

U32 = 2.0 ** -23
EPS_OUT = {torch.bfloat16: 2.0 ** -8, torch.float16: 2.0 ** -11,
           torch.float32: 0.0}


def randn(*shape, seed=0, scale=1.0, dtype=torch.float32):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(tuple(shape), generator=g) * scale).to(dtype)


def _d(t):
    return None if t is None else t.detach().cpu().double()


# ---------------------------------------------------------------- bound ----


def gemm_bound(ref, mag, depth, out_dtype):
    return (EPS_OUT[out_dtype] * ref.abs()
            + 1.01 * (depth + 2) * U32 * mag + 1e-30)


def gemm_violations(out, ref, mag, depth, out_dtype=None):
    """Boolean mask of elements outside the bound (non-finite ones count)."""
    out_dtype = out.dtype if out_dtype is None else out_dtype
    o = _d(out)
    assert o.shape == ref.shape, f"shape {tuple(o.shape)} vs {tuple(ref.shape)}"
    err = (o - ref).abs()
    return ~(err <= gemm_bound(ref, mag, depth, out_dtype))


def assert_gemm_close(out, ref, mag, depth, what="", out_dtype=None):
    out_dtype = out.dtype if out_dtype is None else out_dtype
    bad = gemm_violations(out, ref, mag, depth, out_dtype)
    err = (_d(out) - ref).abs()
    used = (err / gemm_bound(ref, mag, depth, out_dtype)).max().item()
    print(f"ERRBOUND {what} depth={depth} used={used:.4f}")
    if bad.any():
        i = int(torch.nonzero(bad.reshape(-1))[0])
        raise AssertionError(
            f"{what}: {int(bad.sum())}/{bad.numel()} elements outside the "
            f"bound (worst uses {used:.3g}x); first at flat index {i}: out="
            f"{_d(out).reshape(-1)[i].item()!r} ref={ref.reshape(-1)[i].item()!r}"
        )
    return used


# ------------------------------------------------- float64 references ------
# every *_ref returns (ref, mag, depth)


def linear_ref(a, b, bias=None, relu=False):
    """a [..., M, K] @ b [..., N, K]^T (+bias)(+relu)."""
    a, b, bias = _d(a), _d(b), _d(bias)
    ref = a @ b.transpose(-1, -2)
    mag = a.abs() @ b.abs().transpose(-1, -2)
    if bias is not None:
        ref = ref + bias
        mag = mag + bias.abs()
    if relu:
        ref = torch.relu(ref)
    return ref, mag, a.shape[-1]


def nn_ref(a, b):
    """a [..., M, K] @ b [..., K, N]."""
    a, b = _d(a), _d(b)
    return a @ b, a.abs() @ b.abs(), a.shape[-1]


def tn_ref(a, b):
    """a [..., M, I]^T @ b [..., M, J]."""
    a, b = _d(a), _d(b)
    return (a.transpose(-1, -2) @ b, a.abs().transpose(-1, -2) @ b.abs(),
            a.shape[-2])


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def conv_fwd_ref(x, w, bias, stride, pad, relu=False):
    """NHWC x [N,H,W,C] * KRSC w [K,R,S,C] -> [N,HO,WO,K]."""
    x, w, bias = _d(x), _d(w), _d(bias)
    ref = _nhwc(F.conv2d(_nchw(x), _nchw(w), bias, stride, pad))
    mag = _nhwc(F.conv2d(_nchw(x.abs()), _nchw(w.abs()),
                         None if bias is None else bias.abs(), stride, pad))
    if relu:
        ref = torch.relu(ref)
    return ref, mag, w.shape[1] * w.shape[2] * w.shape[3]


def conv_dgrad_ref(dy, w, stride, pad, H, W):
    dy, w = _d(dy), _d(w)
    n, cin = dy.shape[0], w.shape[3]

    def op(g, k):
        return _nhwc(torch.nn.grad.conv2d_input((n, cin, H, W), _nchw(k),
                                                _nchw(g), stride, pad))

    return op(dy, w), op(dy.abs(), w.abs()), w.shape[1] * w.shape[2] * w.shape[0]


def conv_wgrad_ref(dy, x, stride, pad, R, S):
    dy, x = _d(dy), _d(x)
    n, ho, wo, kout = dy.shape

    def op(g, a):
        # one [Kout, M] @ [M, Cin] product per tap over the shifted input
        ap = F.pad(a, (0, 0, pad, pad, pad, pad))
        g2 = g.reshape(-1, kout).t()
        dw = torch.empty(kout, R, S, a.shape[3], dtype=torch.float64)
        for r in range(R):
            for s in range(S):
                sh = ap[:, r:r + stride * (ho - 1) + 1:stride,
                        s:s + stride * (wo - 1) + 1:stride, :]
                dw[:, r, s, :] = g2 @ sh.reshape(-1, a.shape[3])
        return dw

    return op(dy, x), op(dy.abs(), x.abs()), n * ho * wo


def conv_out_hw(h, w, r, stride, pad):
    return (h + 2 * pad - r) // stride + 1, (w + 2 * pad - r) // stride + 1


# ------------------------------------- calibrated (non-GEMM fp32) check ----

CAL_FACTOR = 16.0
CAL_FLOOR = 2.0 ** -20


def rel_err(t, ref):
    ref = _d(ref)
    return ((_d(t) - ref).abs().max() / ref.abs().max().clamp(min=1e-300)).item()


def assert_calibrated(op, gpu, cpu, ref):
    """gpu / cpu / ref: dicts name -> tensor holding the GPU fp32 result, the
    project's CPU fp32 result and the float64 reference of the same op."""
    fails = []
    for name, r in ref.items():
        g, c = gpu[name], cpu[name]
        assert tuple(g.shape) == tuple(r.shape), (op, name, g.shape, r.shape)
        eg, ec = rel_err(g, r), rel_err(c, r)
        tol = max(CAL_FACTOR * ec, CAL_FLOOR)
        ratio = eg / ec if ec > 0 else float("inf") if eg > 0 else 0.0
        print(f"F32CAL {op}.{name} err_gpu={eg:.3e} err_cpu={ec:.3e} "
              f"ratio={ratio:.2f} tol={tol:.3e}")
        if not eg <= tol:
            fails.append(f"{name}: err_gpu {eg:.3e} > tol {tol:.3e} "
                         f"(err_cpu {ec:.3e})")
    assert not fails, f"{op}: " + "; ".join(fails)


# ------------------------------------------------------- poison helper -----


def poison(device, nbytes):
    """Fill a caching-allocator block of ~nbytes with NaN bit patterns and
    free it, so that an op which allocates its own output and leaves part of
    it unwritten returns NaN instead of stale-but-plausible recycled values.
    0xFFFFFFFF words read as NaN in f32, bf16 and fp16 alike."""
    n = max(1, (int(nbytes) + 3) // 4)
    junk = torch.full((n,), -1, dtype=torch.int32, device=device)
    del junk
    torch.cuda.synchronize()
