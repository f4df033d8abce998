"""Record what the reference ``SupervisedLoss`` computes on one small batch, as ``sl_loss_reference.npz`` beside this
file, for ``tests/test_sl_loss_fused.py``.  Needs the reference tree (``APPLESTAR_REFERENCE``, see
``tests/refutil.py``); the test reads only the recorded file.

The batch: b = 6 observations, S = 4 selected-units steps over n = 9 columns, a 3 x 160 location map (C = 480), with
predicted units given so that the IoU is non-zero.  Cases: ``label_smooth`` in {False, True} x ``su_mask`` in
{False, True}.  No ``cross_rank_loss`` case: the reference's all-reduce needs an initialised process group (it raises
"Default process group has not been initialized" without one), so that option is left to the world-1 and the gloo
world-2 tests of ``test_sl_loss_fused.py``.

    python tests/golden/record_sl_loss.py
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
from refutil import import_reference  # noqa: E402

HEADS = ('action_type', 'delay', 'queued', 'selected_units', 'target_unit', 'target_location')
WIDTH = {'action_type': 11, 'delay': 8, 'queued': 2, 'target_unit': 9, 'target_location': 480}
CASES = {'plain': {}, 'su_mask': {'su_mask': True}, 'smooth': {'label_smooth': True},
         'smooth_su_mask': {'label_smooth': True, 'su_mask': True}}


def inputs():
    g = torch.Generator().manual_seed(7)
    b, S, n = 6, 4, 9
    ins = {}
    for h, c in WIDTH.items():
        ins['logits_' + h] = 2 * torch.randn(b, c, generator=g)
        ins['action_' + h] = torch.randint(0, c, (b,), generator=g)
        ins['mask_' + h] = torch.rand(b, generator=g) > 0.3
    ins['mask_action_type'] = torch.ones(b, dtype=torch.bool)
    ins['mask_target_unit'][0] = False
    ins['logits_selected_units'] = 2 * torch.randn(b, S, n, generator=g)
    entity_num = torch.tensor([8, 6, 7, 8, 5, 8])                       # the end flag's column
    su_num = torch.tensor([4, 1, 3, 2, 4, 3])                           # labelled steps, end flag included
    lab = torch.zeros(b, S, dtype=torch.long)
    for i in range(b):
        k = int(su_num[i]) - 1
        lab[i, :k] = torch.randperm(int(entity_num[i]), generator=g)[:k]
        lab[i, k] = entity_num[i]
    lab[4, 1] = lab[4, 0]                                               # a unit labelled twice
    ins['action_selected_units'] = lab
    ins['mask_selected_units'] = torch.tensor([True, True, False, True, True, True])
    preds = lab.clone()                                                 # predictions that overlap the labels in part
    preds[0, 1] = (preds[0, 1] + 1) % 8
    # the reference reads an end flag predicted at step 0 as "no end flag" (sl_loss.py:218) and SupervisedLoss here
    # does not (docs/OPEN_ISSUES.md); no prediction of this batch starts with it
    preds[1] = torch.tensor([3, 6, 0, 0])
    preds[3] = torch.tensor([2, 8, 1, 0])
    preds[5] = torch.tensor([0, 1, 2, 3])                               # no end flag predicted
    ins['preds'] = preds
    ins['selected_units_num'] = su_num
    ins['entity_num'] = entity_num
    return ins


def main():
    import_reference()
    import distar.agent.default.sl_training.sl_loss as rsl
    ins = inputs()
    d = {'in__' + k: v.numpy() for k, v in ins.items()}
    for name, cfg in CASES.items():
        c = {'su_mask': False}
        c.update(cfg)
        loss = rsl.SupervisedLoss(rsl.deep_merge_dicts(rsl.default_config, {'learner': c}))
        logits = {h: ins['logits_' + h].clone() for h in HEADS}
        out = loss.compute_loss(logits, {h: ins['action_' + h].clone() for h in HEADS},
                                {h: ins['mask_' + h].clone() for h in HEADS}, ins['selected_units_num'].clone(),
                                ins['entity_num'].clone(), {'selected_units': ins['preds'].clone()})
        for k, v in out.items():
            d[f'out__{name}__{k}'] = np.asarray(float(v), dtype=np.float64)
    np.savez_compressed(os.path.join(HERE, 'sl_loss_reference.npz'), **d)
    print({k: float(v) for k, v in d.items() if k.startswith('out__')})


if __name__ == '__main__':
    with torch.no_grad():
        main()
