"""The persistent selected-units sampler (csrc/kernels/pointer.hip) against the float64 oracle of
tests/su_sample_oracle.py, at the binding: both kernel forms (1,024 threads, the default, and 256 threads behind
APPLESTAR_SU_WIDE=0), fp32 and bf16 keys, two temperatures, 64 / 7 / 1 steps, rows one below, at and one above every
wave boundary of either form.  Structure exact, every pick within the band of its CDF interval, logits / logp / emb
within ``FACTOR`` times the fp32 host oracle's own error (su_sample_oracle.check)."""
import pytest
import torch

import su_sample_oracle as O
from applestar_amd.ops import native as N

pytestmark = pytest.mark.gpu

FORMS = ('wide', 'narrow')


@pytest.fixture(scope='module')
def C():
    return N.ensure_loaded()


def _run(C, monkeypatch, case, form):
    # read by the launcher on every call; monkeypatch restores it
    monkeypatch.setenv('APPLESTAR_SU_WIDE', '1' if form == 'wide' else '0')
    return O.run_kernel(C, O.inputs(case), case.key_dtype)


@pytest.mark.parametrize('form', FORMS)
@pytest.mark.parametrize('case', O.CASES, ids=O.case_id)
def test_su_sample_matches_oracle(C, monkeypatch, case, form):
    got = _run(C, monkeypatch, case, form)
    assert got['logits'].dtype == torch.float32 and got['results'].dtype == torch.long
    O.check(got, O.inputs(case), form, f'su_sample[{O.case_id(case)},{form}]')


@pytest.mark.parametrize('case', [O.Case('fp32', 0.8, 64, True), O.Case('bf16', 1.0, 64, True)], ids=O.case_id)
def test_su_sample_forms_pick_the_same_units(C, monkeypatch, case):
    """The two forms share every pick and step count, except from a step on whose uniform lies within the band of a
    CDF edge in either form's logits.  From there on the two rows are different sequences: only that first step
    is judged, the rest of the row and its step count are not compared (each form's own row is still held to the
    oracle by the test above), so a near-edge pick at step 0 leaves the whole row uncompared; the print shows it."""
    inp = O.inputs(case)
    wide, narrow = (_run(C, monkeypatch, case, f) for f in FORMS)
    for b in range(inp['key'].shape[0]):
        a, c = wide['results'][b], narrow['results'][b]
        if torch.equal(a, c):
            assert int(wide['su_num'][b]) == int(narrow['su_num'][b]), b
            continue
        t = int(torch.nonzero(a != c)[0])
        n1, _ = O.row_bounds(inp, b)
        lo, u = min(int(a[t]), int(c[t])), float(inp['u'][b, t])
        gaps = [abs(O.cdf_edges(g['logits'][b, t, :n1], lo)[1] - u) for g in (wide, narrow)]
        print(f'row {b} step {t}: picks {int(a[t])} / {int(c[t])}, u - edge {gaps}')
        assert min(gaps) < O.BAND, (b, t, int(a[t]), int(c[t]), gaps)
