"""Helpers to execute the *reference* implementation (read-only source under /root/reference) for
parity tests.  Third-party modules the reference imports but this image lacks (lz4, absl, cv2,
s2clientprotocol, tensorboardX, easydict) are replaced by tiny stubs in tests/refstub; nothing of the
reference is copied.  Tests using this skip when the reference tree is absent (e.g. on GPU boxes).

The small-module parity tests do not need the tree: ``golden(name)`` loads what the reference computed for them,
recorded under ``tests/golden`` by ``tests/golden/record_reference.py``."""
import os
import sys

REF = os.environ.get('APPLESTAR_REFERENCE', '/root/reference')
STUB = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'refstub')
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')


def golden(name):
    """(state_dict, inputs, outputs) of one recorded reference run, as dicts of tensors."""
    import numpy as np
    import torch
    parts = {'sd': {}, 'in': {}, 'out': {}}
    with np.load(os.path.join(GOLDEN, name + '.npz')) as z:
        for k in z.files:
            kind, key = k.split('__', 1)
            parts[kind][key] = torch.from_numpy(z[k])
    return parts['sd'], parts['in'], parts['out']


def reference_available() -> bool:
    return os.path.isdir(os.path.join(REF, 'distar'))


def import_reference():
    import numpy as np
    for name, typ in (('int', int), ('float', float), ('bool', bool)):
        if not hasattr(np, name):
            setattr(np, name, typ)
    for p in (STUB, REF):
        if p not in sys.path:
            sys.path.append(p)
    import distar.agent.default.model.model as ref_model  # noqa
    return ref_model
