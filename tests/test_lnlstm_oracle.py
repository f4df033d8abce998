"""The LN-LSTM oracle (tests/lnlstm_oracle.py) against ``reference.lnlstm_layer`` in float64, and the comparator
against the fp32 host oracle with one defect each: the GPU tests (test_lnlstm_gpu.py) are only as good as these two."""
import pytest
import torch

from applestar_amd.ops import reference as R
from lnlstm_oracle import BWD, CASES, FLOOR, FWD, check, make_inputs, oracle, references

H, T, B = 384, 3, 4         # 48-column owner slices of the split kernels need H = 384; T >= 3 for the step T-2 defect


def _rel(a, b):
    return float((a - b).abs().max()) / max(float(b.abs().max()), 1e-300)


@pytest.mark.parametrize('H,T,B', [(32, 5, 3), (384, 2, 2)])
def test_oracle_matches_reference_layer(H, T, B):
    """xp enters the reference through an identity w_ih and an LN_i whose affine undoes its normalisation exactly,
    so the reference computes the same recurrence from the same xp; its autograd gives every gradient."""
    inp = {k: v.double() for k, v in make_inputs(H, T, B).items()}
    # x = xhat with zero mean and unit biased variance over 4H; LN_i(x I) = xhat * rstd(eps) ~ xhat, scaled back by lni_w
    x = inp['xp'] - inp['xp'].mean(-1, keepdim=True)
    x = (x / x.pow(2).mean(-1, keepdim=True).sqrt()).requires_grad_()
    lni_w = torch.full((4 * H,), (1 + 1e-5) ** 0.5, dtype=torch.float64)
    leaves = [x] + [inp[k].clone().requires_grad_() for k in ('h0', 'c0')] + [torch.eye(4 * H, dtype=torch.float64)] + \
        [inp['w_hh'].clone().requires_grad_(), lni_w, torch.zeros(4 * H, dtype=torch.float64)] + \
        [inp[k].clone().requires_grad_() for k in ('lnh_w', 'lnh_b', 'lnc_w', 'lnc_b')]
    xp = torch.nn.functional.layer_norm(x.detach(), (4 * H,), lni_w, leaves[6])
    r_out, r_h, r_c = R.lnlstm_layer(*leaves)
    want = oracle(**{**inp, 'xp': xp})
    assert set(want) == set(FWD + BWD)
    for k, r in (('out', r_out), ('hT', r_h), ('cT', r_c)):
        assert _rel(want[k], r.detach()) <= 1e-12, k
    assert torch.equal(want['c_all'][0], inp['c0']) and torch.equal(want['c_all'][-1], want['cT'])
    assert torch.equal(want['out'][-1], want['hT'])
    # from xp onward: the same recurrence on an xp that is a leaf
    cell = [t.detach().clone().requires_grad_() for t in (xp, leaves[1], leaves[2], leaves[4], *leaves[7:])]
    h, c, outs = cell[1], cell[2], []
    for t in range(T):
        h, c = R.lnlstm_cell(cell[0][t], h, c, *cell[3:])
        outs.append(h)
    loss = lambda o, h_, c_: (o * inp['dout']).sum() + (h_ * inp['dhT']).sum() + (c_ * inp['dcT']).sum()
    loss(torch.stack(outs, 0), h, c).backward()
    loss(r_out, r_h, r_c).backward()
    for k, g in (('dgates', cell[0].grad), ('dh0', cell[1].grad), ('dc0', cell[2].grad),
                 ('dh0', leaves[1].grad), ('dc0', leaves[2].grad)):
        assert _rel(want[k], g) <= 1e-12, k
    # the parameter gradients, assembled from the oracle's intermediates as ops/native.py assembles the kernels'
    h_prev = torch.cat([inp['h0'][None], want['out'][:-1]], 0)
    mine = {'w_hh': torch.einsum('tbg,tbh->gh', want['dhg'], h_prev),
            'lnh_w': (want['dgates'] * want['xhat_h']).sum((0, 1)), 'lnh_b': want['dgates'].sum((0, 1)),
            'lnc_w': (want['dc_ln'] * want['xhat_c']).sum((0, 1)), 'lnc_b': want['dc_ln'].sum((0, 1))}
    # d(x): dgates through LN_i (the reference's own autograd of that one op)
    x2 = x.detach().clone().requires_grad_()
    torch.nn.functional.layer_norm(x2, (4 * H,), lni_w, leaves[6]).backward(want['dgates'])
    mine['x'] = x2.grad
    for k, g in (('x', x.grad), ('w_hh', leaves[4].grad), ('lnh_w', leaves[7].grad), ('lnh_b', leaves[8].grad),
                 ('lnc_w', leaves[9].grad), ('lnc_b', leaves[10].grad), ('w_hh', cell[3].grad)):
        assert _rel(mine[k], g) <= 1e-12, k
    # the saved statistics are those of the LayerNorms
    hw = h_prev @ inp['w_hh'].t()
    assert _rel(want['rstd_h'], (hw.var(-1, unbiased=False) + 1e-5).rsqrt()) <= 1e-12
    assert _rel(want['gates'], xp.detach() + want['xhat_h'] * inp['lnh_w'] + inp['lnh_b']) <= 1e-12
    assert _rel(want['c_all'][1:], want['xhat_c'] * inp['lnc_w'] + inp['lnc_b']) <= 1e-12


def test_oracle_partial_losses():
    """A missing upstream gradient counts as zero."""
    inp = {k: v.double() for k, v in make_inputs(32, 3, 2).items()}
    a = oracle(**{**inp, 'dout': None, 'dhT': None})
    b = oracle(**{**inp, 'dout': torch.zeros_like(inp['dout']), 'dhT': torch.zeros_like(inp['dhT'])})
    for k in BWD:
        assert torch.equal(a[k], b[k]), k
    assert set(oracle(**{**inp, 'dout': None, 'dhT': None, 'dcT': None})) == set(FWD)


@pytest.mark.parametrize('bf16_w', [False, True], ids=['fp32w', 'bf16w'])
@pytest.mark.parametrize('H,T,B', CASES)
def test_yardstick_stays_at_rounding_level(H, T, B, bf16_w):
    """The inputs of the GPU cases keep the recurrence contractive (make_inputs): the fp32 host oracle's error stays
    within 4 FLOOR of every tensor over all steps, so the bound the kernels meet is a few fp32 ulps and does not depend
    on which way a chaotic sequence happened to round."""
    inp, want, host = references(H, T, B, bf16_w)
    if B >= 2:
        assert not inp['h0'][0].any() and not inp['c0'][0].any() and inp['h0'][1].any()
        assert float(want['rstd_h'][0, 0]) == pytest.approx(1e-5 ** -0.5, rel=1e-12)
    assert all(inp[k].abs().min() > 0 for k in ('dout', 'dhT', 'dcT'))
    if bf16_w:
        assert torch.equal(inp['w_hh'], inp['w_hh'].bfloat16().float())
    for k in FWD + BWD:
        eh = float((host[k].double() - want[k]).abs().max())
        assert eh <= 4 * FLOOR * float(want[k].abs().max()), (k, eh)


@pytest.fixture(scope='module')
def refs():
    inp = make_inputs(H, T, B)
    return inp, oracle(**inp, dtype=torch.float64), oracle(**inp, dtype=torch.float32)


def _with_out_bf(d):
    return {**d, 'out_bf': d['out'].to(torch.bfloat16)}


def test_check_passes_clean_host_run(refs):
    inp, want, host = refs
    assert all(v.dtype == torch.float32 for v in host.values()) and all(v.dtype == torch.float64 for v in want.values())
    rows = check(_with_out_bf(host), want, host, 4, 'clean')
    assert set(rows) == set(FWD + BWD)
    assert all(ek == eh and ek <= bound for ek, eh, bound in rows.values())


def _truncate_bf16(x):
    return (x.contiguous().view(torch.int32) & -65536).view(torch.float32).to(torch.bfloat16)


def _defects(inp):
    run = lambda **kw: oracle(**{**inp, **kw}, dtype=torch.float32)

    def stale_hT():
        d = run()
        d['hT'] = d['out'][T - 2].clone()
        return d

    def stale_slice():
        d = run()
        d['gates'] = d['gates'].clone()
        d['gates'][T - 1, :, 5 * 48:6 * 48] = d['gates'][T - 2, :, 5 * 48:6 * 48]
        return d

    def truncated():
        d = run()
        d['out_bf'] = _truncate_bf16(d['out'])
        return d

    return {'dcT ignored': lambda: run(dcT=torch.zeros_like(inp['dcT'])),
            'hT from step T-2': stale_hT,
            'eps 1e-6 in LN_c': lambda: run(eps_c=1e-6),
            'i and f swapped': lambda: run(gate_order=(1, 0, 2, 3)),
            'stale 48-column slice of gates': stale_slice,
            'out_bf truncated': truncated}


@pytest.mark.parametrize('defect', ['dcT ignored', 'hT from step T-2', 'eps 1e-6 in LN_c', 'i and f swapped',
                                    'stale 48-column slice of gates', 'out_bf truncated'])
def test_check_fails_on_defect(refs, defect):
    inp, want, host = refs
    got = _defects(inp)[defect]()
    got.setdefault('out_bf', got['out'].to(torch.bfloat16))
    with pytest.raises(AssertionError) as e:
        check(got, want, host, 4, defect)
    print(e.value)
    # and for the reason planted, not for the comparator's own bookkeeping
    failed = {r[0] for r in e.value.args[0][1]}
    expect = {'dcT ignored': 'dc0', 'hT from step T-2': 'hT', 'eps 1e-6 in LN_c': 'rstd_c', 'i and f swapped': 'out',
              'stale 48-column slice of gates': 'gates', 'out_bf truncated': 'out_bf'}[defect]
    assert expect in failed, (defect, failed)
    if defect in ('hT from step T-2', 'stale 48-column slice of gates', 'out_bf truncated'):
        assert failed == {expect}
