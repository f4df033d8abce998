"""Step-by-step oracle of the LayerNorm-LSTM recurrence (csrc/kernels/lstm.hip) with every tensor the kernels produce,
the comparator that sets a kernel's error against the oracle's own fp32 rounding, and the binding-level GPU check
built from the two (tests/test_lnlstm_gpu.py; ``python tests/lnlstm_oracle.py --cases H,T,B ...`` runs it in a
process of its own, for the variants the extension reads from the environment once per process).

The cell is ``ops/reference.py: lnlstm_cell`` with the two LayerNorms written out, so that their normalised values
and reciprocal standard deviations, which the forward saves for the backward, can be read:

    gates = xp[t] + LN_h(h W_hh^T);  i, f, g, o = chunk(gates)
    c' = LN_c(sig(f) c + sig(i) tanh(g));  h' = sig(o) tanh(c')

Names are those of the bindings (``lnlstm_fwd`` / ``lnlstm_bwd``)."""
import os
import sys

import torch

EPS = 1e-5
FWD = ('out', 'hT', 'cT', 'c_all', 'gates', 'xhat_h', 'rstd_h', 'xhat_c', 'rstd_c')
BWD = ('dgates', 'dhg', 'dc_ln', 'dh0', 'dc0')
FLOOR = 8 * 2.0 ** -23          # of max|want|: a few fp32 ulps of the tensor's largest value


def _norm(x, eps):
    """(x - mean) * rstd and rstd over the last dim (biased variance), as F.layer_norm before its affine."""
    mu = x.mean(-1, keepdim=True)
    xc = x - mu
    rstd = (xc.pow(2).mean(-1, keepdim=True) + eps).rsqrt()
    return xc * rstd, rstd.squeeze(-1)


def oracle(xp, h0, c0, w_hh, lnh_w, lnh_b, lnc_w, lnc_b, dout=None, dhT=None, dcT=None, dtype=torch.float64,
           eps_h=EPS, eps_c=EPS, gate_order=(0, 1, 2, 3)):
    """The recurrence on the CPU in ``dtype``.  xp [T,B,4H]; w_hh [4H,H] holds the values the kernel multiplies by
    (for a bf16-weight run the caller rounds once and passes the rounded values here and to the kernel).  With
    dout / dhT / dcT the backward of (out*dout).sum() + (hT*dhT).sum() + (cT*dcT).sum() runs too (a missing one
    counts as zero).  ``eps_c`` and ``gate_order`` differ from the cell's only in the comparator's mutation checks.
    Returns a dict of detached tensors: FWD, and BWD when any upstream gradient is given."""
    cast = lambda t: t.detach().to('cpu', dtype).clone()
    xp, h0, c0 = (cast(t).requires_grad_() for t in (xp, h0, c0))
    w_hh, lnh_w, lnh_b, lnc_w, lnc_b = (cast(t) for t in (w_hh, lnh_w, lnh_b, lnc_w, lnc_b))
    T = xp.shape[0]
    assert T >= 1
    h, c = h0, c0
    outs, cs, hws, keep = [], [], [], {k: [] for k in ('gates', 'xhat_h', 'rstd_h', 'xhat_c', 'rstd_c')}
    for t in range(T):
        hw = h @ w_hh.t()
        hw.retain_grad()
        xhat_h, rstd_h = _norm(hw, eps_h)
        gates = xp[t] + (xhat_h * lnh_w + lnh_b)
        chunks = gates.chunk(4, dim=-1)
        i, f, g, o = (chunks[k] for k in gate_order)
        xhat_c, rstd_c = _norm(torch.sigmoid(f) * c + torch.sigmoid(i) * torch.tanh(g), eps_c)
        c = xhat_c * lnc_w + lnc_b
        c.retain_grad()
        h = torch.sigmoid(o) * torch.tanh(c)
        outs.append(h)
        cs.append(c)
        hws.append(hw)
        for k, v in zip(keep, (gates, xhat_h, rstd_h, xhat_c, rstd_c)):
            keep[k].append(v)
    out = torch.stack(outs, 0)
    res = {'out': out, 'hT': h, 'cT': c, 'c_all': torch.stack([c0] + cs, 0)}
    res.update({k: torch.stack(v, 0) for k, v in keep.items()})
    if dout is not None or dhT is not None or dcT is not None:
        loss = 0
        for y, d in ((out, dout), (h, dhT), (c, dcT)):
            if d is not None:
                loss = loss + (y * cast(d)).sum()
        loss.backward()
        res.update(dgates=xp.grad, dhg=torch.stack([v.grad for v in hws], 0),
                   dc_ln=torch.stack([v.grad for v in cs], 0), dh0=h0.grad, dc0=c0.grad)
    return {k: v.detach() for k, v in res.items()}


def check(got, want64, host32, factor=4, what=''):
    """For every tensor of ``got``: max|got - want| <= max(factor * max|host32 - want|, FLOOR * max|want|), where
    host32 is the same oracle run in fp32 - the yardstick is the reference's own rounding, never the kernel.
    ``got['out_bf']``, when present, is
    the bf16 copy of ``got['out']`` and must equal its round-to-nearest-even cast bit for bit.  Prints the three numbers
    per tensor, then raises for all that miss.  Returns {name: (kernel err, host err, bound)}."""
    rows, bad = {}, []
    for k, g in got.items():
        if k == 'out_bf':
            continue
        w = want64[k].double()
        assert g.shape == w.shape, (what, k, tuple(g.shape), tuple(w.shape))
        ek = float((g.double().cpu() - w).abs().max()) if w.numel() else 0.0
        eh = float((host32[k].double() - w).abs().max()) if w.numel() else 0.0
        bound = max(factor * eh, FLOOR * float(w.abs().max()) if w.numel() else 0.0)
        ratio = ek / eh if eh > 0 else float('inf') if ek > 0 else 0.0
        print(f'{what} {k} kernel err {ek:.3e} host err {eh:.3e} bound {bound:.3e} ratio {ratio:.2f}')
        rows[k] = (ek, eh, bound)
        if not ek <= bound:           # a NaN misses too
            bad.append((k, ek, eh, bound))
    if 'out_bf' in got:
        ob, rne = got['out_bf'].cpu(), got['out'].cpu().to(torch.bfloat16)
        assert ob.dtype == torch.bfloat16 and ob.shape == rne.shape, (what, 'out_bf', ob.dtype, tuple(ob.shape))
        n = int((ob.view(torch.int16) != rne.view(torch.int16)).sum())
        print(f'{what} out_bf differs from out.to(bfloat16) in {n} of {ob.numel()} values')
        if n:
            bad.append(('out_bf', n, ob.numel(), 0))
    assert not bad, (what, bad)
    return rows


# ---------------------------------------------------------------------------------------------- the GPU side
# kernel error / fp32 host oracle error allowed by the binding-level check, the project's 4 (test_sl_loss_gpu.py) for
# every tensor: measured on an MI355X the worst ratio over all cases is 2.9 (dgates) where the error is above FLOOR,
# and 5.9 (rstd_h, one scalar at H = 32, T = B = 1, a quarter of FLOOR) below it
FACTOR = 4

# (H, T, B) of the binding-level check, each the smallest shape that reaches the edge it names
CASES = [(384, 1, 1),       # split: the actor's shape, one epoch, one parity
         (384, 1, 16),      # split: largest split batch at T = 1
         (384, 2, 9),       # split: both parities, rows padded to 16 with 7 retired
         (384, 3, 8),       # split: first reuse of a parity buffer, no padding
         (384, 9, 3),       # split: several reuses
         (384, 65, 2),      # split: long sequence (bf16 weights included)
         (384, 1, 17),      # one workgroup per row: first batch size past the split path
         (384, 5, 17),
         (32, 1, 1),        # H = 32: smallest shape
         (32, 64, 5),       # H = 32: the selected-units step count
         (32, 7, 130)]      # H = 32: more rows than two waves of workgroups


def make_inputs(H, T, B, seed=0):
    """CPU fp32 inputs of one case.  With B >= 2 row 0 starts an episode (h0 = c0 = 0: h W = 0 exactly, so
    rstd_h = 1/sqrt(eps), the largest value the backward multiplies by); the other rows carry 0.5 * randn.  The
    upstream gradients are all non-zero.

    The LN_h gain is 0.25 * (1 + 0.1 randn), not the 1 + 0.1 randn of a fresh model.  LN_h makes the recurrent
    term's size independent of W_hh, so this gain alone sets how strongly a step feeds the next, and at 1 a random
    recurrence is chaotic: over 64 steps the fp32 host oracle's error on ``out`` grows to ~300 ulps, max|dgates| to
    ~100x the upstream gradient, and two equally valid fp32 evaluations (hidden units permuted, or another CPU's
    matmul) differ up to 40x in their error on dhg - a yardstick of noise.  At 0.25 the fp32 oracle stays within
    ~1.2x FLOOR on every tensor of every case (test_lnlstm_oracle.py asserts 4x), so the bound is a few fp32 ulps
    of the tensor's largest value, while the kernels run the same code on the same shapes."""
    g = torch.Generator().manual_seed(1000 * H + 10 * T + B + seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    d = dict(xp=rn(T, B, 4 * H), h0=0.5 * rn(B, H), c0=0.5 * rn(B, H), w_hh=rn(4 * H, H) / H ** 0.5,
             lnh_w=0.25 * (1 + 0.1 * rn(4 * H)), lnh_b=0.1 * rn(4 * H), lnc_w=1 + 0.1 * rn(H), lnc_b=0.1 * rn(H),
             dout=rn(T, B, H), dhT=rn(B, H), dcT=rn(B, H))
    if B >= 2:
        d['h0'][0] = 0
        d['c0'][0] = 0
    return d


def run_kernels(C, inp, w_dtype, want_bf16=False, dev='cuda'):
    """lnlstm_fwd, then lnlstm_bwd on the forward's own saved tensors (as ops/native.py does).  ``inp['w_hh']``
    already holds values exact in ``w_dtype``.  Returns the dict of CPU tensors and the forward's tenth value."""
    d = {k: v.to(dev) for k, v in inp.items()}
    w = d['w_hh'].to(w_dtype).contiguous()
    out, hT, cT, c_all, xhat_h, rstd_h, gates, xhat_c, rstd_c, out_bf = C.lnlstm_fwd(
        d['xp'], d['h0'], d['c0'], w.t().contiguous(), d['lnh_w'], d['lnh_b'], d['lnc_w'], d['lnc_b'], EPS, want_bf16)
    dgates, dhg, dc_ln, dh0, dc0 = C.lnlstm_bwd(d['dout'], d['dhT'], d['dcT'], gates, c_all, xhat_c, rstd_c, xhat_h,
                                                rstd_h, w, d['lnh_w'], d['lnc_w'])
    torch.cuda.synchronize()
    got = dict(out=out, hT=hT, cT=cT, c_all=c_all, gates=gates, xhat_h=xhat_h, rstd_h=rstd_h, xhat_c=xhat_c,
               rstd_c=rstd_c, dgates=dgates, dhg=dhg, dc_ln=dc_ln, dh0=dh0, dc0=dc0)
    return {k: v.cpu() for k, v in got.items()}, (None if out_bf is None else out_bf.cpu())


_ORACLES = {}


def references(H, T, B, bf16_w):
    """(inputs, float64 oracle, fp32 host oracle) of a case, computed once per process and left unchanged."""
    key = (H, T, B, bf16_w)
    if key not in _ORACLES:
        inp = make_inputs(H, T, B)
        if bf16_w:
            inp['w_hh'] = inp['w_hh'].bfloat16().float()
        _ORACLES[key] = (inp, oracle(**inp, dtype=torch.float64), oracle(**inp, dtype=torch.float32))
    return _ORACLES[key]


def check_case(C, H, T, B, bf16_w, factor=None):
    """All nine forward and five backward tensors of one case against the oracle, and the exchange's error flag."""
    inp, want, host = references(H, T, B, bf16_w)
    got, _ = run_kernels(C, inp, torch.bfloat16 if bf16_w else torch.float32)
    what = f'lnlstm[{H},{T},{B},{"bf16" if bf16_w else "fp32"}]'
    rows = check(got, want, host, FACTOR if factor is None else factor, what)
    assert int(C.lstm_split_error(0).item()) == 0, 'split LSTM exchange timed out'
    return got, rows


def main(argv):
    import argparse
    p = argparse.ArgumentParser(description=__doc__.split('\n')[0])
    p.add_argument('--cases', nargs='+', required=True, help='H,T,B ...; each runs with fp32 and with bf16 weights')
    args = p.parse_args(argv)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if root not in sys.path:
        sys.path.insert(0, root)
    from applestar_amd.ops import native as N
    C = N.ensure_loaded()
    for case in args.cases:
        H, T, B = (int(v) for v in case.split(','))
        for bf16_w in (False, True):
            check_case(C, H, T, B, bf16_w)
    print('ok')


if __name__ == '__main__':
    main(sys.argv[1:])
