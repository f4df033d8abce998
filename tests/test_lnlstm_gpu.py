"""The LN-LSTM recurrence kernels (csrc/kernels/lstm.hip) against the float64 oracle of tests/lnlstm_oracle.py.

Binding level: every tensor ``lnlstm_fwd`` and ``lnlstm_bwd`` return, on each kernel path (8-workgroup split, one
workgroup per row at H = 384, H = 32), with fp32 and with bf16 weights, at the shapes where each path can go wrong.
The kernel's largest error against float64 may be ``FACTOR`` (lnlstm_oracle.py) times that of the fp32 host oracle.
Then the public wrapper's eleven input gradients under three losses, and the three variants that the extension reads
from the environment, each in a child process."""
import os
import subprocess
import sys

import pytest
import torch

import lnlstm_oracle as O
from applestar_amd.ops import native as N
from applestar_amd.ops import reference as R

pytestmark = pytest.mark.gpu

DEV = 'cuda'
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def C():
    return N.ensure_loaded()


def _is_split(H, B):
    return H == 384 and B <= 16


@pytest.mark.parametrize('bf16_w', [False, True], ids=['fp32w', 'bf16w'])
@pytest.mark.parametrize('H,T,B', O.CASES)
def test_lnlstm_kernels_match_oracle(C, H, T, B, bf16_w):
    got, _ = O.check_case(C, H, T, B, bf16_w)
    # the bf16 copy of out for inference: written by the split path only, and leaves everything else as it was
    inp, want, host = O.references(H, T, B, bf16_w)
    got2, out_bf = O.run_kernels(C, inp, torch.bfloat16 if bf16_w else torch.float32, want_bf16=True)
    if _is_split(H, B):
        assert out_bf is not None and out_bf.dtype == torch.bfloat16
        for k in O.FWD + O.BWD:
            assert torch.equal(got2[k], got[k]), k
        O.check({'out': got2['out'], 'out_bf': out_bf}, want, host, O.FACTOR, f'lnlstm[{H},{T},{B}] want_bf16')
    else:
        assert out_bf is None
    assert int(C.lstm_split_error(0).item()) == 0, 'split LSTM exchange timed out'


# ------------------------------------------------------------------------------------------ the public wrapper
def _wrapper_inputs(H, I, T, B):
    g = torch.Generator().manual_seed(7 * H + T)
    rn = lambda *s: torch.randn(*s, generator=g)
    h0, c0 = 0.5 * rn(B, H), 0.5 * rn(B, H)
    h0[0] = 0
    c0[0] = 0
    ins = [rn(T, B, I), h0, c0, rn(4 * H, I) / I ** 0.5, rn(4 * H, H) / H ** 0.5,
           1 + 0.1 * rn(4 * H), 0.1 * rn(4 * H), 1 + 0.1 * rn(4 * H), 0.1 * rn(4 * H), 1 + 0.1 * rn(H), 0.1 * rn(H)]
    return ins, (rn(T, B, H), rn(B, H), rn(B, H))


_LOSSES = {'out+hT+cT': (True, True, True), 'cT': (False, False, True), 'out': (True, False, False)}


@pytest.mark.parametrize('loss', list(_LOSSES))
@pytest.mark.parametrize('autocast', [False, True], ids=['fp32', 'autocast'])
@pytest.mark.parametrize('H,I,T,B', [(384, 384, 3, 4), (32, 32, 5, 3)])
def test_lnlstm_layer_losses(C, H, I, T, B, autocast, loss):
    """``N.lnlstm_layer`` against ``reference.lnlstm_layer`` in float64 (with the bf16-rounded weight matrices under
    autocast), bounds of test_kernels_gpu.py::test_lnlstm_layer_matches_reference.  'cT' alone reaches
    ``_LNLSTMRecurrence.backward`` with dout and dhT both None."""
    ins, ups = _wrapper_inputs(H, I, T, B)
    dev_in = [t.to(DEV).requires_grad_() for t in ins]
    ref_in = [t.double() for t in ins]
    if autocast:
        for k in (3, 4):
            ref_in[k] = ins[k].bfloat16().double()
    ref_in = [t.requires_grad_() for t in ref_in]
    with torch.autocast('cuda', dtype=torch.bfloat16, enabled=autocast):
        res = N.lnlstm_layer(*dev_in)
    ref = R.lnlstm_layer(*ref_in)
    tol = 5e-2 if autocast else 2e-4
    err = lambda a, b: float((a.detach().double().cpu() - b.detach()).abs().max())
    for k, (a, b, m) in enumerate(zip(res, ref, (1, 1, 4))):
        e = err(a, b)
        print(f'{("out", "hT", "cT")[k]} err {e:.3e} bound {tol * m:.3e}')
        assert e < tol * m
    use = _LOSSES[loss]
    sum(((y * g.to(y.device)).sum() for y, g, u in zip(res, ups, use) if u)).backward()
    sum(((y * g.double()).sum() for y, g, u in zip(ref, ups, use) if u)).backward()
    names = ('x', 'h0', 'c0', 'w_ih', 'w_hh', 'lni_w', 'lni_b', 'lnh_w', 'lnh_b', 'lnc_w', 'lnc_b')
    for n, a, b in zip(names, dev_in, ref_in):
        assert a.grad is not None, n
        scale = max(1.0, float(b.grad.abs().max()))
        e = err(a.grad, b.grad)
        print(f'd{n} err {e:.3e} bound {tol * 4 * scale:.3e}')
        assert e < tol * 4 * scale, n
    torch.cuda.synchronize()
    assert int(C.lstm_split_error(0).item()) == 0, 'split LSTM exchange timed out'


# ------------------------------------------------------------------------------------------ process-level variants
@pytest.mark.parametrize('env', [{'APPLESTAR_LSTM_SPLIT': '0'}, {'APPLESTAR_LSTM_FWD_GRANULE': '1'},
                                 {'APPLESTAR_LSTM_KS': '16'}], ids=lambda e: '-'.join(f'{k}={v}' for k, v in e.items()))
def test_lnlstm_env_variant(env):
    """The unsplit H = 384 kernels at a split batch size, the granule forward exchange and 16 workgroups per row are
    each chosen once per process from the environment: the binding-level check in a fresh child for each."""
    out = subprocess.run([sys.executable, os.path.abspath(O.__file__), '--cases', '384,2,9', '384,3,2'],
                         env=dict(os.environ, **env), capture_output=True, text=True, timeout=120, cwd=ROOT)
    print(out.stdout[-6000:])
    assert out.returncode == 0 and out.stdout.strip().endswith('ok'), (out.returncode, out.stderr[-2000:])
