"""Record what the reference implementation computes for the small-module parity tests, as fixtures
beside this file.  Needs the reference tree (``APPLESTAR_REFERENCE``, see ``tests/refutil.py``); the tests
themselves read only the recorded files.  Each ``.npz`` holds the reference module's random-init weights
(``sd__<key>``), the inputs (``in__<name>``) and the reference's results (``out__<name>``).

    python tests/golden/record_reference.py
"""
import json
import os
import random
import sys
from functools import partial

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from refutil import import_reference  # noqa: E402


def save(name, sd=None, ins=None, outs=None):
    d = {}
    for prefix, tree in (('sd__', sd), ('in__', ins), ('out__', outs)):
        for k, v in (tree or {}).items():
            d[prefix + k] = v.detach().cpu().numpy()
    np.savez_compressed(os.path.join(HERE, name + '.npz'), **d)


def optional_blocks():
    import distar.agent.default.model.module_utils as mu
    import distar.agent.default.model.lstm as rl
    for max_num in (None, 20):
        torch.manual_seed(1)
        ref = mu.AttentionPool(16, 2, 24, max_num=max_num)
        x = torch.randn(4, 7, 16)
        mask = (torch.rand(4, 7, 1) > 0.4)
        num = torch.randint(0, 20, (4,))
        kw = {'num': num} if max_num else {}
        save(f'attention_pool_{max_num}', ref.state_dict(), {'x': x, 'mask': mask, 'num': num},
             {'y': ref(x, mask=mask.clone(), **kw)})
    for method in ('conv-film', 'block-input-film', 'bn-film', 'relu-film', 'block-output-film'):
        torch.manual_seed(2)
        kw = dict(with_cond=[True], with_batchnorm=True, condition_method=method, num_extra_channels=2,
                  extra_channel_freq=2, num_cond_maps=3)
        ref = mu.FiLMedResBlock(8, **kw).eval()
        x = torch.randn(2, 8, 5, 6)
        g, b = torch.randn(2, 8), torch.randn(2, 8)
        ex, cm = torch.randn(2, 2, 5, 6), torch.randn(2, 3, 5, 6)
        save(f'filmed_resblock_{method}', ref.state_dict(), {'x': x, 'g': g, 'b': b, 'ex': ex, 'cm': cm},
             {'y': ref(x, g, b, ex, cm)})
    torch.manual_seed(3)
    ref = mu.LSTM(12, 16, 2, norm_type='LN')
    x = torch.randn(5, 3, 12)
    h0, c0 = torch.randn(2, 3, 16), torch.randn(2, 3, 16)
    ro, rs = ref(x, (h0, c0))
    save('norm_lstm', ref.state_dict(), {'x': x, 'h0': h0, 'c0': c0},
         {'y': ro, 'h': torch.stack([s[0] for s in rs]), 'c': torch.stack([s[1] for s in rs])})
    z = torch.zeros(3, 8)
    for bidirectional in (False, True):
        torch.manual_seed(5)
        ref = rl.script_lstm(6, 8, 2, bidirectional=bidirectional)
        x = torch.randn(4, 3, 6)
        st = [[(z, z), (z, z)] if bidirectional else (z, z) for _ in range(2)]
        save(f'script_lstm_{bidirectional}', ref.state_dict(), {'x': x}, {'y': ref(x, st)[0]})
    torch.manual_seed(6)
    ref = rl.script_lnlstm(6, 8, 2, bidirectional=True)
    x = torch.randn(4, 3, 6)
    st = [[(z, z), (z, z)] for _ in range(2)]
    save('script_lnlstm_bidirectional', ref.state_dict(), {'x': x}, {'y': ref(x, st)[0]})


OPTIM_VARIANTS = [dict(grad_clip_type='clip_value', clip_value=0.5),
                  dict(grad_clip_type='clip_norm', clip_value=1.0),
                  dict(grad_ignore_type='ignore_value', ignore_value=1.5),
                  dict(grad_ignore_type='ignore_value', ignore_value=50.0),
                  dict(grad_ignore_type='ignore_norm', ignore_value=2.0),
                  dict(grad_ignore_type='ignore_norm', ignore_value=100.0)]


def optimizer():
    from distar.ctools.torch_utils.optimizer_util import Adam as RefAdam
    for i, kw in enumerate(OPTIM_VARIANTS):
        g = torch.Generator().manual_seed(1)
        ps = [torch.nn.Parameter(torch.randn(5, 4, generator=g)), torch.nn.Parameter(torch.randn(7, generator=g))]
        for p in ps:
            p.grad = torch.randn(p.shape, generator=g)
        ins = {f'p{j}': p.data.clone() for j, p in enumerate(ps)}
        ins.update({f'g{j}': p.grad.clone() for j, p in enumerate(ps)})
        RefAdam(ps, lr=0.01, betas=(0.0, 0.99), eps=1e-5, **kw).step()
        outs = {f'p{j}': p.data for j, p in enumerate(ps)}
        outs.update({f'g{j}': p.grad for j, p in enumerate(ps)})
        save(f'ref_adam_{i}', None, ins, outs)


def metrics():
    import distar.ctools.torch_utils.metric as m
    rng = random.Random(0)
    g = torch.Generator().manual_seed(0)
    cases = []
    for _ in range(200):
        a = [rng.randint(0, 4) for _ in range(rng.randint(0, 7))]
        b = [rng.randint(0, 4) for _ in range(rng.randint(0, 7))]
        ta, tb = torch.tensor(a, dtype=torch.long), torch.tensor(b, dtype=torch.long)
        c = {'a': a, 'b': b, 'levenshtein': float(m.levenshtein_distance(ta, tb))}
        if len(a) and len(b):
            la = torch.randint(0, 24320, (len(a),), generator=g)
            lb = torch.randint(0, 24320, (len(b),), generator=g)
            c['loc_a'], c['loc_b'] = la.tolist(), lb.tolist()
            c['levenshtein_l2'] = float(m.levenshtein_distance(ta, tb, la, lb, partial(m.l2_distance, spatial_x=160)))
        cases.append(c)
    x = torch.randint(0, 2, (5, 30), generator=g).bool()
    y = torch.randint(0, 2, (5, 30), generator=g).bool()
    h = m.hamming_distance(x, y)
    out = {'cases': cases, 'hamming': {'x': x.int().tolist(), 'y': y.int().tolist(), 'distance': h.tolist(),
                                       'dtype': str(h.dtype)}}
    with open(os.path.join(HERE, 'metric_reference.json'), 'w') as f:
        json.dump(out, f, separators=(',', ':'))


if __name__ == '__main__':
    import_reference()
    with torch.no_grad():
        optional_blocks()
    optimizer()
    metrics()
