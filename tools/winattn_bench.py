"""Time of the fused window attention (ops/csrc/window_attention.hip) at the
four Swin-T stage shapes against the composed route, the only way this op
could be computed before (profiles/r16_window_attention.md).

bf16, batch 128, maps 56/28/14/7 with 3/6/12/24 heads, shift 3 and shift 0.

* fused: ``window_attention`` (two kernels + the dbias reduce).
* composed: ``_window_attention_composed``: torch.roll / permute copies, the
  q/k/v split, bmm_nt, the bias + mask add on the materialised scores, softmax,
  bmm_nn and the way back; every kernel in it predates the fused route.  It is
  the baseline, not the code under test.

Both eagerly, fwd and fwd+bwd (``torch.autograd.grad`` for dqkv and dbias, the
autograd graph built inside every call), device events around CALLS calls
ending in a synchronise, 5 repeats with the cases alternating within every
repeat.  "bytes" is what a route must move by count: the fused route reads qkv
and writes out (fwd), reads qkv and dout and writes dqkv (bwd).

    python tools/winattn_bench.py [--out result.json]
"""

import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_ddp_template_amd.ops import functional as X  # noqa: E402

CALLS, REPEATS = 100, 5
SHAPES = ((128, 56, 3), (128, 28, 6), (128, 14, 12), (128, 7, 24))
SCALE = 32 ** -0.5


def timed(fn, calls):
    """us per call: device events around `calls` back-to-back fn()."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3 / calls


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    result = {"calls_per_window": CALLS, "shapes": {}}
    for n, hw, heads in SHAPES:
        c = heads * 32
        qkv = torch.randn(n, hw, hw, 3 * c, device=dev).to(torch.bfloat16)
        dout = torch.randn(n, hw, hw, c, device=dev).to(torch.bfloat16)
        table = (torch.randn(169, heads, device=dev) * 0.02).to(torch.bfloat16)
        fwd_bytes = (3 * c + c) * n * hw * hw * 2
        bwd_bytes = (3 * c + c + 3 * c) * n * hw * hw * 2
        for shift in (3, 0):
            if hw == 7 and shift:
                continue  # a single window is never shifted

            def run(route, bwd):
                q = qkv.detach().requires_grad_(bwd)
                t = table.detach().requires_grad_(bwd)
                y = route(q, t, heads, shift, SCALE)
                if bwd:
                    torch.autograd.grad(y, (q, t), dout)

            cases = {
                "fused/fwd": lambda: run(X.window_attention, False),
                "fused/fwd_bwd": lambda: run(X.window_attention, True),
                "composed/fwd": lambda: run(X._window_attention_composed, False),
                "composed/fwd_bwd": lambda: run(X._window_attention_composed,
                                                True),
            }
            for fn in cases.values():
                for _ in range(3):
                    fn()
            torch.cuda.synchronize()
            rows = {k: [] for k in cases}
            names = list(cases)
            for rep in range(REPEATS):
                for k in (names if rep % 2 == 0 else names[::-1]):
                    rows[k].append(timed(cases[k], CALLS))
            out = {k: {"us": v} for k, v in rows.items()}
            out["fused/fwd"]["gbps"] = [fwd_bytes / t / 1e3
                                        for t in rows["fused/fwd"]]
            out["fused/fwd_bwd"]["gbps"] = [(fwd_bytes + bwd_bytes) / t / 1e3
                                            for t in rows["fused/fwd_bwd"]]
            for p in ("fwd", "fwd_bwd"):
                out[f"ratio_fused_to_composed/{p}"] = {"ratio": [
                    a / b for a, b in zip(rows[f"fused/{p}"],
                                          rows[f"composed/{p}"])]}
            key = f"{n}x{hw}x{hw}x{heads}h/shift{shift}"
            result["shapes"][key] = out
            for k, v in out.items():
                line = f"{key} {k:32s}"
                if "us" in v:
                    line += " us " + ", ".join(f"{t:.1f}" for t in v["us"])
                if "gbps" in v:
                    line += f"  GB/s {min(v['gbps']):.0f}..{max(v['gbps']):.0f}"
                if "ratio" in v:
                    line += (f" time ratio {min(v['ratio']):.3f}.."
                             f"{max(v['ratio']):.3f}")
                print(line, flush=True)
    print(json.dumps(result), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1)


if __name__ == "__main__":
    main()
