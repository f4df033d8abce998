"""The fp32 3x3 conv weight gradient (C.wgrad_f32 with cin > 0): the per-tap kernels of wgrad_f32.hip (switch 0,
"parent") against the halo-window kernel (conv_wgrad_f32_halo.hip, "halo"), timed alternately in one process.

    python tools/bench_conv_wgrad_f32.py [--pairs 3] [--iters 30] [--out F.jsonl] [--shapes "B,H,W,Cin,Cout;..."]

Per shape: ``pairs`` times (parent, halo), each the median of ``iters`` HIP-event timings of one call (slices +
column reduction, as the learner runs it); one JSON line per measurement and a verdict line per shape: the halo
kernel wins if in every pair its median is below the parent's by more than the spread of the parent's medians.
The default shapes are the learner step's conv weight gradients at B = 390 (spatial encoder) and 384 (location
head): 128 outputs, then the narrow classes (16, 32 and 64 outputs); a shape the halo kernel declines runs the
parent under either switch.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [(390, 19, 20, 128, 128), (384, 19, 20, 128, 128), (390, 38, 40, 64, 128),
          # at most 64 outputs (switch bits 1 and 2: the waves along the reduction rows)
          (384, 76, 80, 64, 32), (390, 76, 80, 32, 64), (384, 38, 40, 128, 64), (390, 19, 20, 32, 32),
          (390, 76, 80, 16, 16), (390, 38, 40, 16, 32)]


def median_us(fn, iters):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ts)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=3)
    ap.add_argument('--iters', type=int, default=30)
    ap.add_argument('--out', default=None)
    ap.add_argument('--shapes', default=None)
    args = ap.parse_args()
    from applestar_amd.ops import native
    C = native.ensure_loaded()
    shapes = SHAPES
    if args.shapes:
        shapes = [tuple(int(v) for v in t.split(',')) for t in args.shapes.split(';')]
    out = open(args.out, 'w') if args.out else None

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        if out:
            out.write(line + '\n')
            out.flush()

    saved = C.conv_wgrad_halo_f32_mode()
    torch.manual_seed(0)
    warm = torch.randn(4096, 4096, device='cuda')      # bring the clocks up before the first timed pair
    for _ in range(50):
        warm @ warm
    torch.cuda.synchronize()
    for B, H, W, ci, co in shapes:
        x = torch.randn(B, H, W, ci, device='cuda').relu()
        dy = torch.randn(B * H * W, co, device='cuda')
        flop = 2.0 * B * H * W * ci * co * 9
        res = {}

        def run(mode):
            C.set_conv_wgrad_halo_f32_mode(mode)
            return C.wgrad_f32(dy, x, ci, True, None)

        for name, mode in (('parent', 0), ('halo', 7)):
            dw, db = run(mode)
            res[name] = (dw.clone(), db.clone())
        diff = float((res['halo'][0] - res['parent'][0]).abs().max())
        med = {'parent': [], 'halo': []}
        for mode in (0, 7):                            # one untimed round each: the shape's first calls allocate
            median_us(lambda m=mode: run(m), args.iters)
        for pair in range(args.pairs):
            for name, mode in (('parent', 0), ('halo', 7)):
                us = median_us(lambda m=mode: run(m), args.iters)
                med[name].append(us)
                emit({'shape': [B, H, W, ci, co], 'kernel': name, 'pair': pair, 'median_us': round(us, 1),
                      'tflops': round(flop / us * 1e-6, 1)})
        spread = max(med['parent']) - min(med['parent'])
        wins = all(p - h > spread for p, h in zip(med['parent'], med['halo']))
        C.set_conv_wgrad_halo_f32_mode(7)
        emit({'shape': [B, H, W, ci, co], 'halo_selected': bool(C.conv_wgrad_f32_halo_selected(co, H, W, ci)),
              'parent_us': [round(v, 1) for v in med['parent']], 'halo_us': [round(v, 1) for v in med['halo']],
              'parent_spread_us': round(spread, 1), 'halo_wins': wins, 'max_abs_diff_dw': diff})
    C.set_conv_wgrad_halo_f32_mode(saved)


if __name__ == '__main__':
    main()
