"""Halo-window fp32 3x3 conv weight gradient (csrc/kernels/conv_wgrad_f32_halo.hip) against float64, and against the
per-tap kernels of wgrad_f32.hip it replaces (switch 0 = the parent's dispatch).

Bound: for every shape the parent's dispatch is run on the same inputs; the new kernel's max error against the
float64 reference must stay within 2x the parent's (both accumulate the same exact bf16 partial products in fp32;
only the summation order differs).  Every input is the contiguous middle of a buffer whose first and last image are
NaN, so a read outside the tensor or a tap that crosses an image edge unmasked shows as a non-finite result.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'
MODES = (0, 1, 2, 4, 7)

# (B, H, W, Cin, Cout)
SHAPES = [
    (5, 19, 20, 128, 128),   # the wide class, slices cutting through images
    (3, 5, 20, 16, 32),      # one chunk
    (2, 7, 40, 48, 64),      # an odd chunk count
    (1, 3, 80, 64, 32),      # the widest window
    (2, 9, 13, 64, 128),     # odd width, R not a multiple of 16 or 32
    (1, 1, 4, 32, 32),       # H = 1
    (1, 2, 1, 32, 64),       # W = 1
    (7, 3, 5, 128, 256),     # two column tiles, the window reaching before pixel 0 and past R
    # the same edge cases in the output class the halo kernel takes (128-multiples)
    (3, 5, 20, 16, 128),     # a chunk half empty
    (2, 7, 40, 48, 128),     # two chunks, the second half empty
    (1, 3, 80, 64, 128),     # the widest window
    (1, 1, 4, 32, 128),      # H = 1, one slice (the out= buffer is the partial)
    (1, 2, 1, 32, 128),      # W = 1
]
DECLINED = (1, 2, 200, 16, 128)   # W past the widest window


def _C():
    from applestar_amd.ops import native
    return native.ensure_loaded()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (NaN-guarded, on the GPU) and the float64 reference, built once per shape."""
    B, H, W, cin, cout = shape
    gen = torch.Generator().manual_seed(1234 + sum(shape))
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
def test_conv_wgrad_halo_matches_fp64(halo_switch, shape):
    C = halo_switch
    for bias in (True, False):
        for use_out in (False, True):
            C.set_conv_wgrad_halo_f32_mode(0)
            pw, pb = _run(C, shape, bias, use_out)
            pw2, pb2 = _run(C, shape, bias, use_out)
            assert torch.equal(pw, pw2) and (pb is None or torch.equal(pb, pb2))      # switch 0, twice
            ew0, eb0 = _errs(shape, pw, pb)
            for mode in MODES[1:]:
                C.set_conv_wgrad_halo_f32_mode(mode)
                dw, db = _run(C, shape, bias, use_out)
                dw2, db2 = _run(C, shape, bias, use_out)
                assert torch.equal(dw, dw2) and (db is None or torch.equal(db, db2))  # run to run
                ew, eb = _errs(shape, dw, db)
                print(f'conv_wgrad_halo {shape} bias={bias} out={use_out} mode={mode}: '
                      f'dw err {ew:.3e} (parent {ew0:.3e})  db err {eb:.3e} (parent {eb0:.3e})')
                assert ew <= 2 * ew0, (mode, ew, ew0)
                assert eb <= 2 * eb0, (mode, eb, eb0)
                if not C.conv_wgrad_f32_halo_selected(shape[4], shape[1], shape[2], shape[3]):
                    assert torch.equal(dw, pw) and (db is None or torch.equal(db, pb))


def test_conv_wgrad_halo_selection(halo_switch):
    C = halo_switch
    C.set_conv_wgrad_halo_f32_mode(7)
    assert C.conv_wgrad_f32_halo_selected(128, 19, 20, 128)
    assert C.conv_wgrad_f32_halo_selected(256, 3, 5, 128)
    assert not C.conv_wgrad_f32_halo_selected(128, 2, 200, 16)      # W past the widest window
    assert not C.conv_wgrad_f32_halo_selected(128, 19, 20, 24)      # Cin % 16
    C.set_conv_wgrad_halo_f32_mode(3)
    assert not C.conv_wgrad_f32_halo_selected(128, 19, 20, 128)
    C.set_conv_wgrad_halo_f32_mode(0)
    assert not C.conv_wgrad_f32_halo_selected(128, 19, 20, 128)


def test_conv_wgrad_halo_declined_shape_is_bit_identical(halo_switch):
    C = halo_switch
    C.set_conv_wgrad_halo_f32_mode(0)
    pw, pb = _run(C, DECLINED, True, False)
    ew0, eb0 = _errs(DECLINED, pw, pb)
    scale = (DECLINED[0] * DECLINED[1] * DECLINED[2]) ** 0.5
    assert ew0 < 1e-4 * scale and eb0 < 1e-4 * scale
    for mode in MODES[1:]:
        C.set_conv_wgrad_halo_f32_mode(mode)
        dw, db = _run(C, DECLINED, True, False)
        assert torch.equal(dw, pw) and torch.equal(db, pb)
