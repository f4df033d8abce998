"""Halo-window fp32 3x3 conv weight gradient for at most 64 outputs (the waves along the reduction rows,
csrc/kernels/conv_wgrad_f32_halo.hip) against float64 and against the per-tap kernels of wgrad_f32.hip (switch 0).

Same construction and bound as test_conv_wgrad_f32_halo_gpu.py: NaN-guarded first and last image, the float64
reference from conv2d_weight, the parent dispatch on the same inputs; the new kernel's max error must stay within 2x
the parent's, finite everywhere and bit-equal run to run.  The shapes are the smallest that reach what the older file
does not: 16 outputs, 16 channels, slices that end in half a stage (64 rows for <= 32 outputs, 32 for <= 64; a
slice's rows are rounded to 32), several slices that cut through images in every output class, W = 80 at 64
outputs, an odd chunk count, 48 outputs (a partly filled second wave column).
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'

# (B, H, W, Cin, Cout)                 R, slices x rows (the last slice's rows)
SHAPES = [
    (3, 7, 13, 16, 16),      # 273 rows: 3 x 96 (81): 1.5 stages a slice; one half-empty chunk, a half-empty tile
    (4, 6, 10, 64, 16),      # 240: 2 x 128 (112); two chunks
    (2, 5, 1, 16, 16),       # W = 1
    (2, 1, 5, 32, 16),       # H = 1
    (2, 9, 13, 96, 32),      # 234: 2 x 128 (106); three chunks
    (6, 19, 20, 32, 32),     # 2280: 18 x 128 (104): the step's 19 x 20 shape, the window wider than a stage
    (2, 2, 80, 48, 64),      # 320: 5 x 64; the widest window, the second chunk half empty
    (3, 5, 7, 32, 64),       # 105: 2 x 64 (41): 1.3 stages in the last slice
    (2, 4, 6, 32, 48),       # 48 outputs
]


def _C():
    from applestar_amd.ops import native
    return native.ensure_loaded()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (NaN-guarded, on the GPU) and the float64 reference, built once per shape."""
    B, H, W, cin, cout = shape
    gen = torch.Generator().manual_seed(4321 + sum(shape))
    xb = torch.full((B + 2, H, W, cin), float('nan'))
    yb = torch.full((B + 2, H, W, cout), float('nan'))
    xb[1:-1] = torch.randn(B, H, W, cin, generator=gen)
    yb[1:-1] = torch.randn(B, H, W, cout, generator=gen)
    ref = torch.nn.grad.conv2d_weight(xb[1:-1].double().permute(0, 3, 1, 2), (cout, cin, 3, 3),
                                      yb[1:-1].double().permute(0, 3, 1, 2), padding=1)   # [Cout, Cin, 3, 3]
    ref_w = ref.permute(0, 2, 3, 1).reshape(cout, 9 * cin).contiguous()                    # [Cout, 3, 3, Cin]
    ref_b = yb[1:-1].double().sum((0, 1, 2))
    xg, yg = xb.to(DEV), yb.to(DEV)
    x, dy = xg[1:-1], yg[1:-1].view(-1, cout)
    assert x.is_contiguous() and dy.is_contiguous()
    return x, dy, ref_w, ref_b, (xg, yg)


def _run(C, shape, bias, use_out):
    x, dy, _, _, _ = _case(shape)
    cin, cout = shape[3], shape[4]
    out = None
    if use_out:
        out = torch.full((cout * 9 * cin + (cout if bias else 0),), float('nan'), device=DEV)
    dw, db = C.wgrad_f32(dy, x, cin, bias, out)
    if use_out:
        assert dw.data_ptr() == out.data_ptr()
    return dw, (db if bias else None)


def _errs(shape, dw, db):
    _, _, ref_w, ref_b, _ = _case(shape)
    assert torch.isfinite(dw).all()
    ew = float((dw.double().cpu() - ref_w).abs().max())
    eb = 0.0
    if db is not None:
        assert torch.isfinite(db).all()
        eb = float((db.double().cpu() - ref_b).abs().max())
    return ew, eb


@pytest.fixture
def halo_switch():
    C = _C()
    saved = C.conv_wgrad_halo_f32_mode()
    assert C.f32_mfma_mode() == 1
    yield C
    C.set_conv_wgrad_halo_f32_mode(saved)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_conv_wgrad_halo_narrow_matches_fp64(halo_switch, shape):
    C = halo_switch
    C.set_conv_wgrad_halo_f32_mode(3)
    assert C.conv_wgrad_f32_halo_selected(shape[4], shape[1], shape[2], shape[3])
    for bias in (True, False):
        for use_out in (False, True):
            C.set_conv_wgrad_halo_f32_mode(0)
            pw, pb = _run(C, shape, bias, use_out)
            ew0, eb0 = _errs(shape, pw, pb)
            C.set_conv_wgrad_halo_f32_mode(3)
            dw, db = _run(C, shape, bias, use_out)
            dw2, db2 = _run(C, shape, bias, use_out)
            assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))      # run to run
            ew, eb = _errs(shape, dw, db)
            print(f'conv_wgrad_halo_narrow {shape} bias={bias} out={use_out}: '
                  f'dw err {ew:.3e} (parent {ew0:.3e})  db err {eb:.3e} (parent {eb0:.3e})')
            assert ew <= 2 * ew0, (ew, ew0)
            assert eb <= 2 * eb0, (eb, eb0)


def test_conv_wgrad_halo_narrow_switch_0_is_the_per_tap_dispatch(halo_switch):
    """Value 0 and a value without the class's bit both run the kernels and the slice count of wgrad_f32.hip: the
    same bits, and other bits than the halo kernel's (whose summation order differs)."""
    C = halo_switch
    for shape, own_bit in (((6, 19, 20, 32, 32), 1), ((2, 2, 80, 48, 64), 2)):
        C.set_conv_wgrad_halo_f32_mode(0)
        pw, pb = _run(C, shape, True, False)
        for mode in (4, 7 & ~own_bit, 0):
            C.set_conv_wgrad_halo_f32_mode(mode)
            dw, db = _run(C, shape, True, False)
            assert torch.equal(dw, pw) and torch.equal(db, pb), mode
        C.set_conv_wgrad_halo_f32_mode(own_bit)
        dw, db = _run(C, shape, True, False)
        assert not torch.equal(dw, pw)


def test_conv_wgrad_halo_narrow_selection(halo_switch):
    C = halo_switch
    C.set_conv_wgrad_halo_f32_mode(7)
    for n in (16, 32, 48, 64):
        assert C.conv_wgrad_f32_halo_selected(n, 19, 20, 32)
        assert C.conv_wgrad_f32_halo_selected(n, 1, 80, 16)
        assert not C.conv_wgrad_f32_halo_selected(n, 2, 81, 16)       # W past the widest window
        assert not C.conv_wgrad_f32_halo_selected(n, 2, 200, 16)
        assert not C.conv_wgrad_f32_halo_selected(n, 19, 20, 24)      # Cin % 16
        assert not C.conv_wgrad_f32_halo_selected(n, 19, 20, 8)
    assert not C.conv_wgrad_f32_halo_selected(96, 19, 20, 32)         # neither <= 64 nor a multiple of 128
    assert not C.conv_wgrad_f32_halo_selected(30, 19, 20, 32)         # not whole column quads
    C.set_conv_wgrad_halo_f32_mode(1)
    assert C.conv_wgrad_f32_halo_selected(16, 19, 20, 32) and C.conv_wgrad_f32_halo_selected(32, 19, 20, 32)
    assert not C.conv_wgrad_f32_halo_selected(48, 19, 20, 32) and not C.conv_wgrad_f32_halo_selected(64, 19, 20, 32)
    assert not C.conv_wgrad_f32_halo_selected(128, 19, 20, 32)
    C.set_conv_wgrad_halo_f32_mode(2)
    assert C.conv_wgrad_f32_halo_selected(48, 19, 20, 32) and C.conv_wgrad_f32_halo_selected(64, 19, 20, 32)
    assert not C.conv_wgrad_f32_halo_selected(16, 19, 20, 32) and not C.conv_wgrad_f32_halo_selected(32, 19, 20, 32)
    for mode in (4, 0):
        C.set_conv_wgrad_halo_f32_mode(mode)
        for n in (16, 32, 48, 64):
            assert not C.conv_wgrad_f32_halo_selected(n, 19, 20, 32)


def test_conv_wgrad_halo_narrow_declines_in_exact_mode(halo_switch):
    """Without the split MFMAs (f32_mfma_mode 0) the halo kernels decline and the result is the per-tap kernels'."""
    C = halo_switch
    shape = (3, 7, 13, 16, 16)
    try:
        C.set_f32_mfma_mode(0)
        C.set_conv_wgrad_halo_f32_mode(7)
        assert not C.conv_wgrad_f32_halo_selected(16, 7, 13, 16)
        assert not C.conv_wgrad_f32_halo_selected(64, 7, 13, 16)
        dw, db = _run(C, shape, True, False)
        C.set_conv_wgrad_halo_f32_mode(0)
        pw, pb = _run(C, shape, True, False)
        assert torch.equal(dw, pw) and torch.equal(db, pb)
    finally:
        C.set_f32_mfma_mode(1)
