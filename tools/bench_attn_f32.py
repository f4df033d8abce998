"""Microbenchmark of the fp32 entity attention at the bench shape, fp32 qkv (variant 23) against qkv as bf16 planes:
forward, backward (dQ + dK/dV) and the QKV GEMM in both output modes.  390 sequences with the synthetic batch's
entity counts (bench.py --batch 6 --unroll 64, seed 0: the first draw of rl_batch's generator), 2 heads x 128,
K = 256.  Method: per item the median of 30 HIP-event timings after an untimed round; three pairs, old and new
alternating; per item the old form's spread over the three medians and the difference of the means.  The extra
bytes the plane GEMM writes count against the attention gain (the `total` row).

    python tools/bench_attn_f32.py
"""
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def median_us(fn, n=30):
    fn()                                     # untimed round
    torch.cuda.synchronize()
    ts = []
    for _ in range(n):
        s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        s.record()
        fn()
        e.record()
        e.synchronize()
        ts.append(s.elapsed_time(e) * 1e3)
    return statistics.median(ts)


def main():
    from applestar_amd.ops import native
    C = native.ensure_loaded()
    H, D, K = 2, 128, 256
    Nn = 3 * H * D
    lens = torch.randint(1, 512, (390,), generator=torch.Generator().manual_seed(0))
    T, mx = int(lens.sum()), int(lens.max())
    cu = torch.cat([torch.zeros(1, dtype=torch.int64), lens.cumsum(0)]).to(torch.int32).cuda()
    torch.manual_seed(0)
    x = torch.randn(T, K, device='cuda')
    w = torch.randn(Nn, K, device='cuda') * 0.05
    b = torch.randn(Nn, device='cuda') * 0.1
    wp = C.presplit_b(w, False, None)
    C.attn_f32_variant(23)
    qkv = C.gemm_f32_psb(x, wp, Nn, K, b, None, 0, 1)
    planes = C.gemm_f32_psb_planes(x, wp, Nn, K, b, 1)
    out, lse = C.varlen_attn_fwd_f32(qkv, cu, mx, H)
    dout = torch.randn_like(out)
    items = {
        'gemm': (lambda: C.gemm_f32_psb(x, wp, Nn, K, b, None, 0, 1), lambda: C.gemm_f32_psb_planes(x, wp, Nn, K, b, 1)),
        'fwd': (lambda: C.varlen_attn_fwd_f32(qkv, cu, mx, H), lambda: C.varlen_attn_fwd_f32(planes, cu, mx, H)),
        'bwd': (lambda: C.varlen_attn_bwd_f32(qkv, out, dout, lse, cu, mx, H),
                lambda: C.varlen_attn_bwd_f32(planes, out, dout, lse, cu, mx, H)),
    }
    res = {'tokens': T, 'sequences': 390, 'max_len': mx}
    for name, (old, new) in items.items():
        o, n = [], []
        for _ in range(3):
            o.append(median_us(old))
            n.append(median_us(new))
        res[name] = {'old_us': [round(v, 1) for v in o], 'new_us': [round(v, 1) for v in n],
                     'old_spread_us': round(max(o) - min(o), 1),
                     'diff_us': round(statistics.mean(n) - statistics.mean(o), 1)}
    res['total'] = {'diff_us': round(sum(res[k]['diff_us'] for k in items), 1)}
    print(json.dumps(res), flush=True)


if __name__ == '__main__':
    main()
