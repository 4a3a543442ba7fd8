"""Time the six stride-2 layers of a ResNet-34 backbone call (layer{2,3,4}.0.conv1 3x3 + .downsample 1x1, 240 x 320 renders) on the
fp32-MFMA direct kernel (mp_conv2d_nhwc, single pass: the plan the backbone would take, split-K tail included) and on the exact-piece
bf16 kernel (mp_conv2d_bf16x9_nhwc); checks that both give the same outputs within CONV_TOL.  One JSON line per layer + a total line.

    python scripts/bench_direct_convs.py --rows 576 --iters 20
"""
import argparse
import json
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parents[1]))

LAYERS = [  # name, Cin, H, W (input), Cout, K, pad
    ("layer2.0.conv1", 64, 60, 80, 128, 3, 1),
    ("layer2.0.downsample", 64, 60, 80, 128, 1, 0),
    ("layer3.0.conv1", 128, 30, 40, 256, 3, 1),
    ("layer3.0.downsample", 128, 30, 40, 256, 1, 0),
    ("layer4.0.conv1", 256, 15, 20, 512, 3, 1),
    ("layer4.0.downsample", 256, 15, 20, 512, 1, 0),
]


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=576)
    ap.add_argument("--iters", type=int, default=20)
    a = ap.parse_args()
    from megapose6d_amd import engine as eng

    N = a.rows
    ws = torch.empty(12 << 20, device="cuda")   # the backbone's split-K scratch
    tot = {"fp32": 0.0, "bf16x9": 0.0}
    g = torch.Generator(device="cuda").manual_seed(0)
    for name, Cin, H, W, Cout, K, pad in LAYERS:
        Ho, Wo = (H + 2 * pad - K) // 2 + 1, (W + 2 * pad - K) // 2 + 1
        xb = eng.padded_nhwc(N, H, W, Cin, 1, "cuda")
        eng.padded_view(xb, N, H, W, Cin, 1)[:] = torch.randn(N, H, W, Cin, device="cuda", generator=g)
        w = (torch.randn(Cout, Cin, K, K) * (2.0 / (Cin * K * K)) ** 0.5).numpy()
        wp = torch.from_numpy(eng.conv_pack_weights(w, Cin, None)).cuda()
        wb = torch.from_numpy(eng.conv_bf16x9_pack_weights(w, Cin, None)).cuda()
        bias = torch.randn(Cout, device="cuda") * 0.1
        ys = {k: eng.padded_nhwc(N, Ho, Wo, Cout, 1, "cuda") for k in tot}
        runs = {
            "fp32": lambda y: eng.conv2d_nhwc(xb, N, H, W, Cin, 1, wp, bias, Cout, K, 2, pad, y, 1, relu=True, splitk_ws=ws),
            "bf16x9": lambda y: eng.conv2d_bf16x9_nhwc(xb, N, H, W, Cin, 1, wb, bias, Cout, K, 2, pad, y, 1, relu=True),
        }
        ms = {}
        for k in ("fp32", "bf16x9", "fp32", "bf16x9"):   # alternated; the second round is kept
            for _ in range(3):
                runs[k](ys[k])
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            for _ in range(a.iters):
                runs[k](ys[k])
            t1.record()
            torch.cuda.synchronize()
            ms[k] = t0.elapsed_time(t1) / a.iters
        scale = ys["fp32"].abs().max().item()
        diff = (ys["fp32"] - ys["bf16x9"]).abs().max().item()
        for k in tot:
            tot[k] += ms[k]
        flops = 2.0 * N * Ho * Wo * Cout * Cin * K * K
        print(json.dumps({"layer": name, "rows": N, "fp32_ms": round(ms["fp32"], 4), "bf16x9_ms": round(ms["bf16x9"], 4),
                          "speedup": round(ms["fp32"] / ms["bf16x9"], 3), "bf16x9_alg_tflops": round(flops / ms["bf16x9"] * 1e-9, 1),
                          "bf16x9_mfma_busy_est": round(9 * flops / ms["bf16x9"] * 1e-9 / 2500.0, 3),
                          "max_abs_diff_over_scale": diff / max(scale, 1e-30)}), flush=True)
        assert diff <= 2e-5 * max(1.0, scale), (name, diff, scale)
        del xb, wp, wb, ys
    print(json.dumps({"total_fp32_ms": round(tot["fp32"], 4), "total_bf16x9_ms": round(tot["bf16x9"], 4),
                      "speedup": round(tot["fp32"] / tot["bf16x9"], 3)}), flush=True)


if __name__ == "__main__":
    main()
