"""The halo-window fp32 3x3 conv (csrc/kernels/conv3x3_f32_halo.hip) vs float64 on the CPU.

The kernel stages each 128-pixel tile's input once per 16-channel chunk as a pre-split window and reads every tap
from it; rows outside the image are redirected to a zero slot.  Checked here: every epilogue the learner uses on
shapes that cross image and tensor boundaries, no leak from neighbouring images or neighbouring memory, run-to-run
bit identity, the fall-back of ``conv3x3_f32_psb`` and the agreement of its two dispatches.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda'

# (B, H, W, Cin, Cout)
SHAPES = [
    (3, 5, 20, 16, 32),        # three tiles, ragged last tile, tiles crossing image boundaries, one chunk
    (2, 7, 40, 48, 64),        # odd chunk count
    (1, 3, 80, 64, 32),        # widest window, four chunks
    (2, 4, 80, 32, 64),        # the spatial encoder's class
    (1, 2, 20, 128, 64),       # M < 128: window before pixel 0 and past M
    (5, 19, 20, 128, 128),     # the 128-output instantiation
    (2, 9, 13, 64, 256),       # two column tiles, odd width
]
UNSUPPORTED = (1, 2, 200, 16, 32)     # wider than the widest window: conv3x3_f32_psb keeps the ring kernel
EPILOGUES = ['bias_relu', 'res', 'drelu', 'epi2']


def _C():
    from applestar_amd.ops import native as N
    return N.ensure_loaded()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (CPU, fp32) and the float64 conv without epilogue, computed once per shape and never modified."""
    B, H, W, Ci, Co = shape
    g = torch.Generator().manual_seed(1234 + sum(shape))
    t = {'x': torch.randn(B, H, W, Ci, generator=g),
         'w': torch.randn(Co, 3, 3, Ci, generator=g) / (9 * Ci) ** 0.5,
         'bias': torch.randn(Co, generator=g),
         'res': torch.randn(B, H, W, Co, generator=g),
         'res2': torch.randn(1, H, W, Co, generator=g),
         'mask': torch.randn(B, H, W, Co, generator=g)}
    t['conv'] = torch.nn.functional.conv2d(t['x'].double().permute(0, 3, 1, 2), t['w'].double().permute(0, 3, 1, 2),
                                           padding=1).permute(0, 2, 3, 1).contiguous()
    return t


def _reference(t, epi):
    conv = t['conv']
    if epi == 'bias_relu':
        return (conv + t['bias'].double()).relu()
    if epi == 'res':
        return conv + t['bias'].double() + t['res'].double()
    if epi == 'drelu':
        return torch.where(t['res'] > 0, conv, torch.zeros_like(conv))
    ref = conv + t['res'].double()
    ref[:1] += t['res2'].double()
    return torch.where(t['mask'] > 0, ref, torch.zeros_like(ref))


def _run(fn, t, epi, x=None):
    """fn: _C.conv3x3_f32_halo or _C.conv3x3_f32_psb (same signature)."""
    C = _C()
    d = {k: v.to(DEV) for k, v in t.items() if k != 'conv'}
    x = d['x'] if x is None else x
    Co = d['w'].shape[0]
    ws = C.presplit_b(d['w'].reshape(Co, -1).contiguous())
    if epi == 'bias_relu':
        return fn(x, ws, Co, d['bias'], None, None, None, 1)
    if epi == 'res':
        return fn(x, ws, Co, d['bias'], d['res'], None, None, 0)
    if epi == 'drelu':
        return fn(x, ws, Co, None, d['res'], None, None, 4)
    return fn(x, ws, Co, None, d['res'], d['res2'], d['mask'], 0)


def _check(got, ref):
    err = (got.double().cpu() - ref).abs().max().item()
    bound = 2e-5 * max(1.0, ref.abs().max().item())
    print('err', err, 'bound', bound)
    assert err < bound, (err, bound)


@pytest.mark.parametrize('epi', EPILOGUES)
@pytest.mark.parametrize('shape', SHAPES)
def test_halo_matches_fp64(shape, epi):
    C = _C()
    B, H, W, Ci, Co = shape
    assert C.conv3x3_f32_halo_supported(H, W, Ci, Co)
    t = _case(shape)
    _check(_run(C.conv3x3_f32_halo, t, epi), _reference(t, epi))


@pytest.mark.parametrize('epi', EPILOGUES)
def test_unsupported_width_falls_back(epi):
    """W = 200 is wider than the widest window: with every class switched on, conv3x3_f32_psb still matches."""
    C = _C()
    B, H, W, Ci, Co = UNSUPPORTED
    assert not C.conv3x3_f32_halo_supported(H, W, Ci, Co)
    t = _case(UNSUPPORTED)
    before = C.conv_halo_f32_mode()
    C.set_conv_halo_f32_mode(7)
    try:
        got = _run(C.conv3x3_f32_psb, t, epi)
    finally:
        C.set_conv_halo_f32_mode(before)
    _check(got, _reference(t, epi))
    with pytest.raises(RuntimeError):
        _run(C.conv3x3_f32_halo, t, epi)


def test_no_leak_from_neighbouring_image():
    """A NaN-filled middle image: the taps of images 0 and 2 that fall outside their image read zeros."""
    C = _C()
    shape = SHAPES[0]
    t = _case(shape)
    x = t['x'].to(DEV).clone()
    x[1] = float('nan')
    got = _run(C.conv3x3_f32_halo, t, 'bias_relu', x=x).cpu()
    ref = _reference(t, 'bias_relu')
    for b in (0, 2):
        assert torch.isfinite(got[b]).all()
        _check(got[b], ref[b])


def test_no_leak_from_neighbouring_memory():
    """x as the interior of a larger NaN-filled allocation: window rows before pixel 0 and past M read zeros."""
    C = _C()
    shape = SHAPES[0]
    B, H, W, Ci, Co = shape
    t = _case(shape)
    big = torch.full((B + 2, H, W, Ci), float('nan'), device=DEV)
    big[1:B + 1] = t['x'].to(DEV)
    x = big[1:B + 1]
    assert x.is_contiguous() and x.data_ptr() != big.data_ptr()
    got = _run(C.conv3x3_f32_halo, t, 'bias_relu', x=x)
    assert torch.isfinite(got).all()
    _check(got, _reference(t, 'bias_relu'))


@pytest.mark.parametrize('shape', [SHAPES[1], SHAPES[3], SHAPES[5]])
def test_two_launches_bit_identical(shape):
    C = _C()
    t = _case(shape)
    a = _run(C.conv3x3_f32_halo, t, 'epi2')
    b = _run(C.conv3x3_f32_halo, t, 'epi2')
    assert torch.equal(a, b)


@pytest.mark.parametrize('entry', ['conv3x3_f32_psb', 'conv3x3_f32_v2', 'conv3x3_f32_halo'])
def test_presplit_entries_validate_operands(entry):
    """The three pre-split entry points share one operand check: each refuses short planes, a strided x, a bias or
    residual of the wrong size and Cin = 8 with a message that starts with its own name, and still runs the valid
    call."""
    C = _C()
    shape = (1, 2, 20, 16, 32)
    B, H, W, Ci, Co = shape
    t = _case(shape)
    d = {k: v.to(DEV) for k, v in t.items() if k != 'conv'}
    ws = C.presplit_b(d['w'].reshape(Co, -1).contiguous())
    fn = getattr(C, entry)
    extra = (2,) if entry == 'conv3x3_f32_v2' else ()       # the ring entry's variant

    def call(x=d['x'], ws=ws, co=Co, bias=d['bias'], res=d['res']):
        return fn(x, ws, co, bias, res, None, None, 0, *extra)

    x8 = torch.zeros(B, H, W, 8, device=DEV)
    w8 = torch.zeros(Co, 3, 3, 8, device=DEV)
    bad = {
        'short wsplit': dict(ws=ws[:-1].contiguous()),
        'strided x': dict(x=torch.zeros(B, H, W, 2 * Ci, device=DEV)[..., ::2]),
        'bias Cout + 1': dict(bias=torch.zeros(Co + 1, device=DEV)),
        'res of another size': dict(res=torch.zeros(B, H, W - 1, Co, device=DEV)),
        'Cin = 8': dict(x=x8, ws=C.presplit_b(w8.reshape(Co, -1).contiguous())),
    }
    for what, kw in bad.items():
        with pytest.raises(RuntimeError) as e:
            call(**kw)
        assert str(e.value).startswith(entry + ':'), (what, str(e.value))
    _check(call(), _reference(t, 'res'))


@pytest.mark.parametrize('shape', SHAPES)
def test_psb_switch_on_and_off_agree(shape):
    """conv3x3_f32_psb with the halo kernel switched off (the ring kernel) and on: same split products, another
    summation order."""
    C = _C()
    t = _case(shape)
    before = C.conv_halo_f32_mode()
    try:
        C.set_conv_halo_f32_mode(0)
        off = _run(C.conv3x3_f32_psb, t, 'epi2')
        C.set_conv_halo_f32_mode(7)
        on = _run(C.conv3x3_f32_psb, t, 'epi2')
    finally:
        C.set_conv_halo_f32_mode(before)
    err = (on - off).abs().max().item()
    bound = 1e-5 * max(1.0, off.abs().max().item())
    print('err', err, 'bound', bound)
    assert err <= bound, (err, bound)
