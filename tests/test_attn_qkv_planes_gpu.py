"""fp32 attention on qkv kept as bf16 planes: the plane output of the pre-split GEMM (gemm_f32_psb_planes), the
plane forms of the attention kernels (attention_f32.hip) and the fused QKV-linear + attention node
(ops.qkv_attention).  Everything here is an exactness check: the planes are the truncation split of the fp32
result, and the plane kernels run the products of the default fp32-qkv variant in the same order."""
import pytest
import torch

from applestar_amd import ops
from applestar_amd.models.transformer import TransformerLayer
from applestar_amd.ops import native as N

pytestmark = pytest.mark.gpu

DEV = 'cuda'
H, D = 2, 128
HD3 = 3 * H * D


@pytest.fixture(scope='module', autouse=True)
def _load():
    N.ensure_loaded()


@pytest.fixture
def C():
    """The extension in its default modes (split MFMA, attention variant 23), restored afterwards."""
    c = N.ensure_loaded()
    mode, var = c.f32_mfma_mode(), c.attn_f32_variant(23)
    c.set_f32_mfma_mode(1)
    yield c
    c.set_f32_mfma_mode(mode)
    c.attn_f32_variant(var)


def _trunc(v):
    return (v.view(torch.int32) & -65536).view(torch.float32)


def _split3(y):
    """The truncation split of csrc/split_mfma.h in torch: three bf16 tensors with p0 + p1 + p2 == y."""
    p0 = _trunc(y)
    r1 = y - p0
    p1 = _trunc(r1)
    p2 = _trunc(r1 - p1)
    return [p.to(torch.bfloat16) for p in (p0, p1, p2)]      # low 16 bits are zero: the casts are exact


def _bits(t):
    return t.contiguous().view(torch.int16)


def _cu(lens):
    return torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=DEV)


def _count(monkeypatch, C, names):
    calls = {n: 0 for n in names}
    for n in names:
        f = getattr(C, n)

        def wrap(*a, _f=f, _n=n, **kw):
            calls[_n] += 1
            return _f(*a, **kw)
        monkeypatch.setattr(C, n, wrap)
    return calls


# ------------------------------------------------------------------ 1. the plane GEMM is exact
@pytest.mark.parametrize('variant', [1, 0])
@pytest.mark.parametrize('M', [1, 129, 700])
def test_plane_gemm_is_the_split_of_the_fp32_gemm(C, M, variant):
    torch.manual_seed(M)
    K, Nn = 256, HD3
    x = torch.randn(M, K, device=DEV)
    w = torch.randn(Nn, K, device=DEV) * 0.1
    b = torch.randn(Nn, device=DEV)
    wp = C.presplit_b(w, False, None)
    y = C.gemm_f32_psb(x, wp, Nn, K, b, None, 0, variant)
    sentinel = -7.0
    buf = torch.full((3 * M * Nn + 5 * Nn,), sentinel, device=DEV, dtype=torch.bfloat16)
    ret = C.gemm_f32_psb_planes(x, wp, Nn, K, b, variant, buf)
    assert ret.data_ptr() == buf.data_ptr()
    planes = buf[:3 * M * Nn].view(3, M, Nn)
    total = (planes[0].float() + planes[1].float()) + planes[2].float()
    assert torch.equal(total.view(torch.int32), y.view(torch.int32))
    for got, want in zip(planes, _split3(y)):
        assert torch.equal(_bits(got), _bits(want))
    assert bool((buf[3 * M * Nn:] == sentinel).all()), 'rows past M were written'
    fresh = C.gemm_f32_psb_planes(x, wp, Nn, K, b, variant)
    assert fresh.shape == (3, M, Nn) and torch.equal(_bits(fresh), _bits(planes))


# ------------------------------------------------------------------ 2. attention equals the default variant
def _attn_both(C, qkv, planes, cu, mx, dout):
    out, lse = C.varlen_attn_fwd_f32(qkv, cu, mx, H)
    dqkv = C.varlen_attn_bwd_f32(qkv, out, dout, lse, cu, mx, H)
    pout, plse = C.varlen_attn_fwd_f32(planes, cu, mx, H)
    pdqkv = C.varlen_attn_bwd_f32(planes, pout, dout, plse, cu, mx, H)
    return (out, lse, dqkv), (pout, plse, pdqkv)


@pytest.mark.parametrize('lens', [[1, 64, 65, 200, 511], [37], [128, 3, 300], [31, 32, 33, 63]])
@pytest.mark.parametrize('score_scale', [0.5, 2.0])
def test_plane_attention_equals_default_variant(C, lens, score_scale):
    """out, lse and dqkv of the plane kernels against variant 23 on the fp32 qkv: no form reorders a sum, so the
    comparison is torch.equal."""
    torch.manual_seed(11)
    T = sum(lens)
    cu = _cu(lens)
    qkv = torch.randn(T, HD3, device=DEV) * score_scale
    planes = torch.stack(_split3(qkv))
    dout = torch.randn(T, H * D, device=DEV)
    ref, got = _attn_both(C, qkv, planes, cu, max(lens), dout)
    for name, a, b in zip(('out', 'lse', 'dqkv'), got, ref):
        assert torch.equal(a, b), (name, (a - b).abs().max().item())


# ------------------------------------------------------------------ 3. nothing leaks across sequences
@pytest.mark.parametrize('lens', [[20, 40, 75], [75, 40, 20]], ids=['short_before', 'midblock_before'])
def test_plane_attention_does_not_read_the_neighbour(C, lens):
    """Sequence 1 is NaN before the planes are made: its neighbours (one shorter than a 32-row image block, one
    ending in the middle of a block) must come out finite and exactly as without the NaN sequence."""
    torch.manual_seed(5)
    T, cu, mx = sum(lens), _cu(lens), max(lens)
    qkv = torch.randn(T, HD3, device=DEV)
    dout = torch.randn(T, H * D, device=DEV)
    bad = qkv.clone()
    bad[lens[0]:lens[0] + lens[1]] = float('nan')
    keep = torch.ones(T, dtype=torch.bool, device=DEV)
    keep[lens[0]:lens[0] + lens[1]] = False

    def run(q):
        planes = torch.stack(_split3(q))
        out, lse = C.varlen_attn_fwd_f32(planes, cu, mx, H)
        return out, lse, C.varlen_attn_bwd_f32(planes, out, dout, lse, cu, mx, H)

    (o0, l0, g0), (o1, l1, g1) = run(qkv), run(bad)
    for name, a, b in (('out', o1[keep], o0[keep]), ('lse', l1[:, keep], l0[:, keep]), ('dqkv', g1[keep], g0[keep])):
        assert bool(torch.isfinite(a).all()), name
        assert torch.equal(a, b), name


# ------------------------------------------------------------------ 4. one transformer layer, switch on vs off
def _layer_run(layer, x0, cu, mx, g):
    x = x0.clone().requires_grad_()
    h = x * 1.0                      # a non-leaf input: the residual gradient travels through the GradLink
    y = layer.forward_packed(h, cu, mx)
    loss = (y * g).sum()
    # as the trainer does: weight gradients of single-consumer weights are deferred to a side stream, and
    # autograd.grad hands the nodes' own tensors back (an accumulating .backward() may copy them too early)
    N.defer_begin(DEV, loss)
    try:
        grads = torch.autograd.grad(loss, [x] + list(layer.parameters()))
    finally:
        N.defer_end(DEV)
    torch.cuda.synchronize()
    return [y.detach()] + list(grads)


@pytest.mark.parametrize('route', ['as_routed', 'psb_forced'])
def test_layer_switch_on_equals_off(C, monkeypatch, route):
    """TransformerLayer.forward_packed at T = 300, APPLESTAR_ATTN_QKV_PLANES on against off: output, input
    gradient (with the GradLink residual) and every parameter gradient (deferred dW) bit for bit.  At 300 rows the
    linears are below the pre-split GEMM's tile-count rule, so `as_routed` keeps the separate ops under both
    settings; `psb_forced` lifts that rule (for both settings alike) so that the fused node is what runs."""
    torch.manual_seed(3)
    if route == 'psb_forced':
        monkeypatch.setattr(N, '_psb_ok', lambda M, Nn, K: N.GEMM_PSB and C.gemm_f32_psb_supported(M, Nn, K))
    calls = _count(monkeypatch, C, ['gemm_f32_psb_planes'])
    lens = [100, 37, 163]
    layer = TransformerLayer(256, D, 1024, H, 2, 'post').to(DEV)
    x0 = torch.randn(sum(lens), 256, device=DEV)
    g = torch.randn(sum(lens), 256, device=DEV)
    monkeypatch.setattr(N, 'ATTN_QKV_PLANES', False)
    off = _layer_run(layer, x0, _cu(lens), max(lens), g)
    assert calls['gemm_f32_psb_planes'] == 0
    monkeypatch.setattr(N, 'ATTN_QKV_PLANES', True)
    on = _layer_run(layer, x0, _cu(lens), max(lens), g)
    assert calls['gemm_f32_psb_planes'] == (1 if route == 'psb_forced' else 0)
    assert len(on) == len(off) == 2 + len(list(layer.parameters()))
    for i, (a, b) in enumerate(zip(on, off)):
        assert a is not None and torch.equal(a, b), i


# ------------------------------------------------------------------ 5. who takes the new path
def _qkv_problem(device, dtype=torch.float32):
    torch.manual_seed(9)
    lens = [500, 400, 300, 200]                    # 1400 rows: above the pre-split GEMM's tile-count rule
    T = sum(lens)
    x = torch.randn(T, 256, device=device, dtype=dtype)
    w = torch.nn.Parameter((torch.randn(HD3, 256, device=device) * 0.05).to(dtype))
    b = torch.nn.Parameter(torch.randn(HD3, device=device).to(dtype))
    cu = torch.tensor([0] + list(torch.tensor(lens).cumsum(0)), dtype=torch.int32, device=device)
    return x, w, b, cu, max(lens)


def _fused_and_separate(x, w, b, cu, mx):
    res = []
    for fused in (True, False):
        xx = x.clone().requires_grad_()
        w.grad = b.grad = None
        if fused:
            y = ops.qkv_attention(xx, w, b, cu, mx, H, D)
        else:
            y = ops.varlen_attention(ops.linear(xx, w, b), cu, mx, H, D)
        y.float().square().sum().backward()
        res.append([y.detach(), xx.grad, w.grad.clone(), b.grad.clone()])
    return res


def test_fused_node_runs_in_split_mode_and_equals_the_separate_ops(C, monkeypatch):
    calls = _count(monkeypatch, C, ['gemm_f32_psb_planes', 'gemm_f32_psb'])
    fused, sep = _fused_and_separate(*_qkv_problem(DEV))
    assert calls['gemm_f32_psb_planes'] == 1
    for i, (a, b) in enumerate(zip(fused, sep)):
        assert torch.equal(a, b), i


@pytest.mark.parametrize('case', ['exact_mfma', 'bf16', 'cpu', 'no_grad', 'switch_off'])
def test_fallbacks_take_the_separate_ops(C, monkeypatch, case):
    calls = _count(monkeypatch, C, ['gemm_f32_psb_planes'])
    if case == 'exact_mfma':
        C.set_f32_mfma_mode(0)
    if case == 'switch_off':
        monkeypatch.setattr(N, 'ATTN_QKV_PLANES', False)
    x, w, b, cu, mx = _qkv_problem('cpu' if case == 'cpu' else DEV, torch.bfloat16 if case == 'bf16' else torch.float32)
    if case == 'no_grad':
        with torch.no_grad():
            a = ops.qkv_attention(x, w, b, cu, mx, H, D)
            r = ops.varlen_attention(ops.linear(x, w, b), cu, mx, H, D)
        assert torch.equal(a, r)
    else:
        fused, sep = _fused_and_separate(x, w, b, cu, mx)
        for i, (a, r) in enumerate(zip(fused, sep)):
            assert torch.equal(a, r), i
    assert calls['gemm_f32_psb_planes'] == 0
