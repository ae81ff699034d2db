"""CPU: the inputs of the weighted GPU cases can tell right from wrong (tests/obs_weights_util.py), and the one check every entry
point applies to `obs_weights` before it launches anything (`capi.dense_obs_weights`)."""
import pytest
import torch

from nlt_amd import capi as C
from oracle import nlt_oracle as O
import obs_weights_util as U


@pytest.mark.parametrize('c', U.FORWARD, ids=U.case_id)
def test_forward_cases_are_sensitive_to_the_weights(c):
    kw, batch, nn, w = U.forward_inputs(c)
    om = O.OracleModel(**kw)
    _, dist = U.assert_sensitive(lambda wv: U.oracle_forward(om, batch, nn, wv), w, U.FORWARD_BARS, U.case_id(c))
    print(U.case_id(c), {k: round(v, 3) for k, v in dist.items()})


@pytest.mark.parametrize('c', U.TRAIN, ids=U.case_id)
def test_train_cases_are_sensitive_to_the_weights(c):
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    _, dist = U.assert_sensitive(lambda wv: U.oracle_train(c, wv)[2], U.forward_inputs(c)[3], U.TRAIN_BARS, U.case_id(c))
    print(U.case_id(c), {k: round(v, 3) for k, v in dist.items()})


def test_weight_matrices():
    for n, k in ((1, 1), (2, 1), (3, 2), (2, 3), (3, 4)):
        U.check_weights(O.synth_obs_weights(n, k), n, k)
    assert O.synth_obs_weights(2, 3).tolist() == [[0., 2., -1.], [1.5, .25, 3.]]


def test_dense_obs_weights_accepts_what_the_reference_s_reshape_accepts():
    dev = torch.device('cpu')
    assert C.dense_obs_weights(None, 3, 2, dev) is None
    w = O.synth_obs_weights(3, 2)
    assert torch.equal(C.dense_obs_weights(w, 3, 2, dev), w)
    wide = O.synth_obs_weights(3, 4)
    for view in (wide[:, :2], wide[:, :2].t().contiguous().t(), w.reshape(3, 1, 1, 1, 2), w.reshape(3, 2, 1)):
        d = C.dense_obs_weights(view, 3, 2, dev)
        assert d.is_contiguous() and tuple(d.shape) == (3, 2) and d.dtype == torch.float32 and torch.equal(d, w)
    assert not wide[:, :2].is_contiguous() and not wide[:, :2].t().contiguous().t().is_contiguous()


@pytest.mark.parametrize('bad', ['float64', 'int32', 'k_only', 'one_column_more', 'flat_one_more', 'transposed_shape', 'list', 'meta'])
def test_dense_obs_weights_refuses_the_rest(bad):
    n, k = 3, 2
    w = O.synth_obs_weights(n, k)
    arg = {'float64': w.double(), 'int32': w.to(torch.int32), 'k_only': w[0], 'one_column_more': O.synth_obs_weights(n, k + 1),
           'flat_one_more': torch.zeros(n * k + 1), 'transposed_shape': w.t(), 'list': w.tolist(),
           'meta': torch.empty((n, k), device='meta')}[bad]
    with pytest.raises(ValueError, match='obs_weights') as e:
        C.dense_obs_weights(arg, n, k, torch.device('cpu'))
    if torch.is_tensor(arg):                                  # the message names what it got
        assert str(tuple(arg.shape)) in str(e.value) and str(arg.dtype) in str(e.value) and str(arg.device) in str(e.value)
