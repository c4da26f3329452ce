"""Per-stage times of the transformer MLP at the ViT-B/16 batch-256 shapes
(M = 50432; 768 -> 3072 -> 768), three routes each: the library GEMM plus the
separate elementwise pass, the in-house 256x256 kernel plus the same pass, and
the epilogue-fused kind (gemm_nt_epi).  Device events around ITERS calls,
REPS repeats, routes interleaved; prints min / median / max in ms per call.

    python tools/mlp_gelu_bench.py        (profiles/r18_mlp_gelu.md)
"""

import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from pytorch_ddp_template_amd.ops.native import native  # noqa: E402

M, C, H = 50432, 768, 3072
ITERS, REPS = 20, 7


def main():
    assert torch.cuda.is_available(), "needs the GPU"
    ext, dev, bf = native(), "cuda:0", torch.bfloat16
    g = torch.Generator(device=dev).manual_seed(0)

    def rnd(*s, scale=1.0):
        return (torch.randn(*s, device=dev, generator=g) * scale).to(bf)

    x, dout, res = rnd(M, C), rnd(M, C), rnd(M, C)
    w1, b1 = rnd(H, C, scale=C ** -0.5), rnd(H)
    w2, b2 = rnd(C, H, scale=H ** -0.5), rnd(C)
    y, gact = ext.gemm_nt_epi(x, w1, b1, "bias_gelu", None)
    w2t = ext.transpose2d(w2)

    stages = {
        "fc1 fwd (bias+gelu)": {
            "library+pass": lambda: ext.gelu_fwd(F.linear(x, w1, b1)),
            "inhouse+pass": lambda: ext.gelu_fwd(
                ext.gemm_nt(x, w1, b1, False, False)),
            "fused": lambda: ext.gemm_nt_epi(x, w1, b1, "bias_gelu", None),
        },
        "fc2 fwd (bias+residual)": {
            "library+pass": lambda: res + F.linear(gact, w2, b2),
            "inhouse+pass": lambda: res + ext.gemm_nt(
                gact, w2, b2, False, False),
            "fused": lambda: ext.gemm_nt_epi(gact, w2, b2, "bias_res", res),
        },
        "fc2 dgrad (x gelu')": {
            "library+pass": lambda: ext.gelu_bwd(dout @ w2, y),
            "inhouse+pass": lambda: ext.gelu_bwd(
                ext.gemm_nt(dout, w2t, None, False, False), y),
            "fused": lambda: ext.gemm_nt_epi(dout, w2t, None, "mul_dgelu", y),
        },
    }
    for stage, routes in stages.items():
        times = {k: [] for k in routes}
        for f in routes.values():
            for _ in range(3):
                f()
        for _ in range(REPS):
            for k, f in routes.items():
                t0, t1 = (torch.cuda.Event(enable_timing=True) for _ in "ab")
                t0.record()
                for _ in range(ITERS):
                    f()
                t1.record()
                torch.cuda.synchronize()
                times[k].append(t0.elapsed_time(t1) / ITERS)
        for k, v in times.items():
            print(f"{stage:26s} {k:13s} min {min(v):.3f} med "
                  f"{statistics.median(v):.3f} max {max(v):.3f} ms", flush=True)


if __name__ == "__main__":
    main()
