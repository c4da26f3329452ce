"""Kernel time of the depthwise conv kernels (ops/csrc/dwconv.hip) at the four
ConvNeXt-T stage shapes against torch's grouped conv, the only path this op
could take before (profiles/r14_dwconv.md).

bf16, batch 128, 7x7 pad 3, maps 56/28/14/7 with C 96/192/384/768.

* dw_fwd / dw_dgrad / dw_wgrad: the three bindings.  Timed twice: "graph" is
  device events around REPLAYS replays of a captured graph of LAUNCHES calls
  (no host launch rate in it), "eager" is device events around LAUNCHES *
  REPLAYS plain calls on the current stream.
* lib_fwd: ``F.conv2d(groups=C)`` on channels-last tensors; lib_fwd_bwd: the
  same forward plus ``torch.autograd.grad`` for dx and dw, the autograd graph
  built inside every call.  Timed eagerly ONLY, and set against the eager
  dw figures (fwd against fwd, the sum of the three against fwd_bwd).  The
  library is never captured here: an autograd graph recorded outside a capture
  and differentiated inside it runs its backward nodes on the stream the
  forward used (the default stream), which is illegal while another stream
  captures and takes the process down; see bench.py's capture recipe.

5 repeats, the cases of a shape alternating within every repeat.  GB/s is
against the bytes a kernel must move: one read and one write of the map (fwd,
dgrad), two reads (wgrad); the weights are noise.

    python tools/dwconv_bench.py [--out result.json]
"""

import argparse
import json
import os
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from pytorch_ddp_template_amd.ops.native import native  # noqa: E402

LAUNCHES, REPLAYS, REPEATS = 10, 50, 5
SHAPES = ((128, 56, 96), (128, 28, 192), (128, 14, 384), (128, 7, 768))
R, PAD = 7, 3


def timed(fn, calls):
    """us per call: device events around `calls` back-to-back fn()."""
    t0 = torch.cuda.Event(enable_timing=True)
    t1 = torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(calls):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) * 1e3


def capture(fn):
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(3):
            fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        for _ in range(LAUNCHES):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "needs the GPU"
    dev = torch.device("cuda:0")
    ext = native()
    calls = LAUNCHES * REPLAYS
    result = {"calls_per_window": calls, "shapes": {}}
    for n, hw, c in SHAPES:
        x = torch.randn(n, hw, hw, c, device=dev).to(torch.bfloat16)
        dy = torch.randn(n, hw, hw, c, device=dev).to(torch.bfloat16)
        w = (torch.randn(c, R, R, 1, device=dev) * 0.1).to(torch.bfloat16)
        # the library's view of the same data: NCHW shape, channels-last memory
        xl = x.permute(0, 3, 1, 2)
        dyl = dy.permute(0, 3, 1, 2)
        wl = w.permute(0, 3, 1, 2).contiguous()
        assert xl.is_contiguous(memory_format=torch.channels_last)

        def lib_fwd():
            return F.conv2d(xl, wl, None, 1, PAD, groups=c)

        def lib_fwd_bwd():
            xr = xl.detach().requires_grad_(True)
            wr = wl.detach().requires_grad_(True)
            y = F.conv2d(xr, wr, None, 1, PAD, groups=c)
            return torch.autograd.grad(y, (xr, wr), dyl)

        nbytes = 2 * x.numel() * 2
        dw_cases = {
            "dw_fwd": lambda: ext.dwconv2d_fwd(x, w, None, PAD),
            "dw_dgrad": lambda: ext.dwconv2d_dgrad(dy, w, PAD, hw, hw),
            "dw_wgrad": lambda: ext.dwconv2d_wgrad(dy, x, PAD, R),
        }
        eager = dict(dw_cases, lib_fwd=lib_fwd, lib_fwd_bwd=lib_fwd_bwd)
        graphs = {name: capture(fn) for name, fn in dw_cases.items()}
        for fn in eager.values():
            for _ in range(3):
                fn()
        torch.cuda.synchronize()
        rows = {f"{name}/graph": [] for name in graphs}
        rows.update({f"{name}/eager": [] for name in eager})
        names = list(rows)
        for rep in range(REPEATS):
            for key in (names if rep % 2 == 0 else names[::-1]):
                name, mode = key.split("/")
                if mode == "graph":
                    g = graphs[name]
                    g.replay()
                    rows[key].append(timed(g.replay, REPLAYS) / calls)
                else:
                    eager[name]()
                    rows[key].append(timed(eager[name], calls) / calls)
        out = {k: {"us": v} for k, v in rows.items()}
        for k, v in out.items():
            if k.startswith("dw_") or k.startswith("lib_fwd/"):
                v["gbps"] = [nbytes / t / 1e3 for t in v["us"]]
        dw_all = [sum(t) for t in zip(*(rows[f"{k}/eager"] for k in dw_cases))]
        out["fwd_ratio_dw_to_lib/eager"] = {"ratio": [
            a / b for a, b in zip(rows["dw_fwd/eager"], rows["lib_fwd/eager"])]}
        out["fwd_bwd_ratio_dw_to_lib/eager"] = {"ratio": [
            a / b for a, b in zip(dw_all, rows["lib_fwd_bwd/eager"])]}
        key = f"{n}x{hw}x{hw}x{c}"
        result["shapes"][key] = out
        for k, v in out.items():
            line = f"{key} {k:30s}"
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
