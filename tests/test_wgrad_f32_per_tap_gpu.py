"""The per-tap conv kernels of csrc/kernels/wgrad_f32.hip (the dispatch with the halo kernels switched off) against
float64, on images smaller than one stage's rows: the only case where the row walker (csrc/wgrad_tile.h) passes over
more than one image per advance, and where slices end inside images and inside a stage.

Bound: the project's own for every fp32 kernel, in both product modes: err < 2e-5 * max(1, |ref|.max()) for dW and
db (a plain fp32 conv2d_weight sits at about 1 % of it on these shapes; one missing or leaked product is O(1)).
Every input is the contiguous middle of a buffer whose first and last image are NaN, so a read outside the tensor or
a tap that crosses an image edge unmasked shows as a non-finite result.
"""
import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = 'cuda'

# (B, H, W, Cin, Cout): R = B H W between 50 and 273
SHAPES = [
    (40, 1, 5, 16, 32),
    (40, 5, 1, 16, 64),
    (37, 2, 3, 16, 128),
    (50, 1, 1, 16, 32),      # one slice
    (9, 3, 5, 4, 128),       # K = 36: the 64-wide K tile, a tap boundary every 4 columns
    (9, 3, 5, 4, 64),
    (3, 7, 13, 32, 136),     # a second, mostly empty N tile
]


def _C():
    from applestar_amd.ops import native
    return native.ensure_loaded()


@functools.lru_cache(maxsize=None)
def _case(shape):
    """Inputs (NaN-guarded, on the GPU) and the float64 reference, built once per shape."""
    B, H, W, cin, cout = shape
    gen = torch.Generator().manual_seed(77 + sum(shape))
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


@pytest.fixture(params=['split', 'exact'])
def per_tap(request):
    """The per-tap dispatch (halo kernels off) in both product modes of the fp32 kernels; both restored."""
    C = _C()
    mode, halo = C.f32_mfma_mode(), C.conv_wgrad_halo_f32_mode()
    C.set_f32_mfma_mode(1 if request.param == 'split' else 0)
    C.set_conv_wgrad_halo_f32_mode(0)
    yield C
    C.set_conv_wgrad_halo_f32_mode(halo)
    C.set_f32_mfma_mode(mode)


@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_wgrad_f32_per_tap_small_images_match_fp64(per_tap, shape):
    C = per_tap
    x, dy, ref_w, ref_b, _ = _case(shape)
    cin, cout = shape[3], shape[4]
    assert not C.conv_wgrad_f32_halo_selected(cout, shape[1], shape[2], cin)
    dw, db = C.wgrad_f32(dy, x, cin, True)
    dw2, db2 = C.wgrad_f32(dy, x, cin, True)
    assert torch.equal(dw, dw2) and torch.equal(db, db2)
    assert torch.isfinite(dw).all() and torch.isfinite(db).all()
    ew = float((dw.double().cpu().reshape(cout, 9 * cin) - ref_w).abs().max())
    eb = float((db.double().cpu() - ref_b).abs().max())
    bw = 2e-5 * max(1.0, float(ref_w.abs().max()))
    bb = 2e-5 * max(1.0, float(ref_b.abs().max()))
    print(f'wgrad_f32 per-tap {shape}: dw err {ew:.3e} (bound {bw:.3e})  db err {eb:.3e} (bound {bb:.3e})')
    assert ew < bw, (ew, bw)
    assert eb < bb, (eb, bb)
