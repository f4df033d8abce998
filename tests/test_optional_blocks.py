"""Optional network blocks (models/optional.py): numerics vs the reference modules (CPU, fp32; the reference's
random-init weights, the inputs and its outputs are recorded under tests/golden), plus self-consistency checks."""
import pytest
import torch

from refutil import golden
from applestar_amd.models import optional as O


def test_attention_pool_prefix_matches_sequential_masks():
    torch.manual_seed(0)
    for max_num in (None, 65):
        ap = O.AttentionPool(32, 2, 64, max_num=max_num)
        B, N, S = 3, 9, 5
        key = torch.randn(B, N, 32)
        labels = torch.stack([torch.randperm(N)[:S] for _ in range(B)])  # distinct, as in the head
        new = torch.rand(B, S) > 0.3
        new[0] = False  # an empty selection: uniform softmax over all tokens
        got = ap.prefix(key, labels, new)
        for i in range(S):
            m = torch.zeros(B, N)
            for b in range(B):
                for j in range(i + 1):
                    if new[b, j]:
                        m[b, labels[b, j]] = 1
            exp = ap(key, num=m.sum(1), mask=m.unsqueeze(2))
            torch.testing.assert_close(got[:, i], exp, atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize('max_num', [None, 20])
def test_attention_pool_matches_reference(max_num):
    sd, ins, want = golden(f'attention_pool_{max_num}')
    ours = O.AttentionPool(16, 2, 24, max_num=max_num)
    ours.load_state_dict(sd, strict=True)
    kw = {'num': ins['num']} if max_num else {}
    torch.testing.assert_close(ours(ins['x'], mask=ins['mask'], **kw), want['y'], atol=1e-5, rtol=1e-5)


@pytest.mark.parametrize('method', ['conv-film', 'block-input-film', 'bn-film', 'relu-film', 'block-output-film'])
def test_filmed_resblock_matches_reference(method):
    sd, ins, want = golden(f'filmed_resblock_{method}')
    kw = dict(with_cond=[True], with_batchnorm=True, condition_method=method, num_extra_channels=2,
              extra_channel_freq=2, num_cond_maps=3)
    ours = O.FiLMedResBlock(8, **kw).eval()
    ours.load_state_dict(sd, strict=True)
    got = ours(ins['x'], ins['g'], ins['b'], ins['ex'], ins['cm'])
    torch.testing.assert_close(got, want['y'], atol=1e-5, rtol=1e-5)


def test_norm_lstm_matches_reference():
    sd, ins, want = golden('norm_lstm')
    ours = O.NormLSTM(12, 16, 2, norm_type='LN')
    ours.load_state_dict(sd, strict=True)
    oo, (oh, oc) = ours(ins['x'], (ins['h0'], ins['c0']))
    torch.testing.assert_close(oo, want['y'], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(oh, want['h'], atol=1e-5, rtol=1e-5)
    torch.testing.assert_close(oc, want['c'], atol=1e-5, rtol=1e-5)


def test_pytorch_lstm_state_formats():
    torch.manual_seed(4)
    m = O.get_lstm('pytorch', 6, 8, 2)
    x = torch.randn(4, 3, 6)
    out, (h, c) = m(x, None)
    assert out.shape == (4, 3, 8) and h.shape == (2, 3, 8)
    per_sample = [None, (h[:, 1:2], c[:, 1:2]), None]
    out2, listed = m(x, per_sample, list_next_state=True)
    assert len(listed) == 3 and listed[0][0].shape == (2, 1, 8)


@pytest.mark.parametrize('bidirectional', [False, True])
def test_script_lstm_matches_reference(bidirectional):
    sd, ins, want = golden(f'script_lstm_{bidirectional}')
    ours = O.script_lstm(6, 8, 2, bidirectional=bidirectional)
    ours.load_state_dict(sd, strict=True)
    z = torch.zeros(3, 8)
    st = [[(z, z), (z, z)] if bidirectional else (z, z) for _ in range(2)]
    oo, _ = ours(ins['x'], st)
    torch.testing.assert_close(oo, want['y'], atol=1e-5, rtol=1e-5)


def test_bidirectional_lnlstm_matches_reference():
    sd, ins, want = golden('script_lnlstm_bidirectional')
    ours = O.script_lnlstm(6, 8, 2, bidirectional=True)
    ours.load_state_dict(sd, strict=True)
    z = torch.zeros(3, 8)
    st = [[(z, z), (z, z)] for _ in range(2)]
    oo, _ = ours(ins['x'], st)
    torch.testing.assert_close(oo, want['y'], atol=1e-4, rtol=1e-4)


def test_block_builders_key_layout():
    blk = O.conv2d_block(4, 8, 3, 1, 1, activation='relu', norm_type='BN')
    assert list(blk.state_dict())[:2] == ['0.weight', '0.bias']
    assert blk(torch.randn(2, 4, 5, 5)).shape == (2, 8, 5, 5)
    blk = O.conv2d_block(4, 8, 3, 1, 1, pad_type='reflect')
    assert blk(torch.randn(2, 4, 5, 5)).shape == (2, 8, 5, 5)
    d = O.deconv2d_block(8, 4, 4, 2, 1, activation='relu')
    assert d(torch.randn(2, 8, 5, 5)).shape == (2, 4, 10, 10)
    f = O.fc_block2(16, 1, gain=0.1, norm_type='LN')
    assert float(f[0].bias.detach().abs().sum()) == 0.0
    assert O.build_normalization('BN', 2) is torch.nn.BatchNorm2d
    assert O.build_normalization('LN', 1) is torch.nn.LayerNorm
    sbn = O.build_normalization('SyncBN', 2)(8)
    assert sbn(torch.randn(3, 8, 4, 4)).shape == (3, 8, 4, 4)  # no process group -> plain BN
    with pytest.raises(KeyError):
        O.build_normalization('XX')
