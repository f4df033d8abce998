"""Per-site cost of the deterministic mode: each ordered kernel beside the default (atomic / torch) form it replaces,
at the bench shapes (6 x 64 trajectories = 390 observations, up to 512 entities / units), one JSON line per site.

    python tools/bench_deterministic.py [--iters 20]

Times are medians of HIP-event timings of one call (forward, or forward + backward where the site is a backward);
``default_ms`` is the mode off, ``ordered_ms`` the mode on.
"""
import argparse
import json
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from applestar_amd import ops  # noqa: E402
from applestar_amd.ops import native as N  # noqa: E402

DEV = 'cuda'


def timed(fn, iters):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts)


def both(name, fn, iters, **meta):
    res = {}
    for key, flag in (('default_ms', False), ('ordered_ms', True)):
        prev = N.set_deterministic(flag)
        try:
            res[key] = round(timed(fn, iters), 4)
        finally:
            N.set_deterministic(prev)
    print(json.dumps({'site': name, **meta, **res}), flush=True)


def spatial_sites(iters, B=390, H=152, W=160, Nn=512):
    from applestar_amd.lib.features import SPATIAL_ONE_HOT, EFFECT_KEYS
    sp = {'height_map': torch.randint(0, 256, (B, H, W), device=DEV, dtype=torch.uint8)}
    for k, n in SPATIAL_ONE_HOT:
        sp[k] = torch.randint(0, n, (B, H, W), device=DEV, dtype=torch.uint8)
    for k in EFFECT_KEYS:
        sp[k] = torch.randint(0, H * W, (B, 8), device=DEV, dtype=torch.int16)
    ex, ey = torch.randint(0, W, (B, Nn), device=DEV), torch.randint(0, H, (B, Nn), device=DEV)
    en = torch.randint(1, Nn, (B,), device=DEV)
    w, b = torch.randn(32, 24, device=DEV) * 0.3, torch.randn(32, device=DEV) * 0.1
    for prec in ('fp32', 'bf16'):
        rows = torch.randn(B, Nn, 32, device=DEV).to(torch.float32 if prec == 'fp32' else torch.bfloat16)

        def run(pool):
            with torch.no_grad(), torch.autocast('cuda', dtype=torch.bfloat16, enabled=prec == 'bf16'):
                (N.spatial_embed_pool if pool else N.spatial_embed)(sp, rows, ex, ey, en, w, b)
        both('spatial_embed', lambda: run(False), iters, precision=prec)
        both('spatial_embed_pool', lambda: run(True), iters, precision=prec)


def scatter_site(iters, B=390, U=512, C=8, H=152, W=160):
    x = torch.randint(0, W, (B, U), device=DEV, dtype=torch.uint8)
    y = torch.randint(0, H, (B, U), device=DEV, dtype=torch.uint8)
    g = torch.randn(B, C, H, W, device=DEV).contiguous(memory_format=torch.channels_last)
    for dtype in (torch.float32, torch.bfloat16):
        proj = torch.randn(B, U, C, device=DEV).to(dtype).requires_grad_()

        def run():
            proj.grad = None
            ops.scatter_connection(proj, x, y, H, W).backward(g.to(dtype))
        both('value_scatter_connection fwd+bwd', run, iters, precision=str(dtype).split('.')[-1])


def gather_site(iters, B=384, N1=513, S=64, C=32):
    labels = torch.randint(0, N1, (B, S), device=DEV)
    g = torch.randn(B, S, C, device=DEV)
    for dtype in (torch.float32, torch.bfloat16):
        key = torch.randn(B, N1, C, device=DEV).to(dtype).requires_grad_()

        def run():
            key.grad = None
            ops.gather_steps(key, labels).backward(g.to(dtype))
        both('selected_units gather_steps fwd+bwd', run, iters, precision=str(dtype).split('.')[-1])


def table_sites(iters):
    C = N.ensure_loaded()
    for U, V, D in ((390 * 512, 260, 8), (390 * 512, 2, 8)):
        src = torch.randn(U, D, device=DEV)
        idx = torch.randint(0, V, (U,), device=DEV)
        both('table_grad', lambda: C.table_grad(src, idx, V, N.deterministic()), iters, U=U, V=V, D=D)
    for U, V, D in ((390, 5, 32), (390 * 20, 128, 64)):
        table = torch.randn(V, D, device=DEV)
        idx = torch.randint(0, V, (U,), device=DEV)
        out = C.embed_relu_fwd(table, idx)
        dout = torch.randn(U, D, device=DEV)
        both('embed_relu_bwd', lambda: C.embed_relu_bwd(dout, out, idx, V, N.deterministic()), iters, U=U, V=V, D=D)


def bo_site(iters, B=390):
    from applestar_amd.models.encoders import BeginningBuildOrderEncoder
    bo = torch.randint(0, 174, (B, 20), device=DEV)
    loc = torch.randint(0, 152 * 160, (B, 20), device=DEV)
    g = torch.randn(B, 64, device=DEV)
    for prec in ('fp32', 'bf16'):
        enc = BeginningBuildOrderEncoder(64).to(DEV)
        if prec == 'bf16':
            for i, p in enumerate(enc.fused_params()):
                if not (i >= 2 and (i - 2) % 12 in (0, 1, 6, 7)):
                    p.data = p.data.to(torch.bfloat16)
        out = enc(bo, loc)
        both('bo_encoder backward', lambda: out.float().backward(g, retain_graph=True), iters, precision=prec)


def rl_loss_site(iters, T=64, B=6, F=1):
    C = N.ensure_loaded()
    r = lambda *s: torch.randn(*s, device=DEV)  # noqa: E731
    alp, blp, ent, kl = -r(6, T, B).abs(), -r(6, T, B).abs(), r(6, T, B).abs(), r(6, T, B).abs()
    hm, v, rew, wm, at = torch.ones(6, T, B, device=DEV), r(F, T + 1, B), r(F, T, B), torch.ones(F, T, B, device=DEV), \
        torch.ones(T, B, device=DEV)
    sc = torch.ones(4 * F + 28, device=DEV)
    both('rl_loss', lambda: C.rl_loss(alp, blp, hm, ent, kl, v, rew, wm, at, sc, 0, False, N.deterministic()), iters,
         T=T, B=B, F=F)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    args = ap.parse_args()
    N.ensure_loaded()
    torch.manual_seed(0)
    for site in (spatial_sites, scatter_site, gather_site, table_sites, bo_site, rl_loss_site):
        site(args.iters)
        torch.cuda.empty_cache()


if __name__ == '__main__':
    main()
