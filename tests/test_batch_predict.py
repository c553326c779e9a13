"""CPU checks of the batched posterior predictors' boundary (lfm_batch_posterior_f64,
dis_project_amd.predict): the packing helpers, the exported symbol and the NULL-context
rejection. The GPU parity is tests/test_gpu_batch_predict.py."""

import numpy as np
import pytest

from dis_project_amd import _lib
from dis_project_amd import predict as P


def test_pack_and_unpack_round_trip_on_ragged_m():
    rng = np.random.default_rng(0)
    genes = [4, 5, 1, 3]
    ms = [8, 5, 7, 30]
    ts = [rng.uniform(0, 13, (m, 3)) for m in ms]
    t, m = P.pack_test_inputs(ts, genes)
    assert m.dtype == np.int64 and m.tolist() == ms
    assert t.shape == (sum(ms), 3) and t.flags.c_contiguous and t.dtype == np.float64
    off = 0
    for a, k in zip(ts, ms):
        np.testing.assert_array_equal(t[off:off + k], a)
        off += k
    mean = rng.standard_normal(sum(ms))
    var = rng.standard_normal(sum(ms))
    cov = rng.standard_normal(sum(k * k for k in ms))
    out = P.unpack_outputs(m, mean, var, cov)
    assert [o[0].shape for o in out] == [(k,) for k in ms]
    assert [o[2].shape for o in out] == [(k, k) for k in ms]
    np.testing.assert_array_equal(np.concatenate([o[0] for o in out]), mean)
    np.testing.assert_array_equal(np.concatenate([o[1] for o in out]), var)
    np.testing.assert_array_equal(np.concatenate([o[2].reshape(-1) for o in out]), cov)
    # row-major blocks: element (1, 0) of problem 1's covariance
    assert out[1][2][1, 0] == cov[ms[0] ** 2 + ms[1]]
    only_var = P.unpack_outputs(m, mean, var)
    assert all(o[2] is None for o in only_var)
    only_cov = P.unpack_outputs(m, mean, None, cov)
    assert all(o[1] is None for o in only_cov)


def test_shared_test_inputs_are_repeated_per_problem():
    t1 = np.arange(60.0).reshape(20, 3)
    t, m = P.pack_test_inputs(t1, [4, 5, 2])
    assert m.tolist() == [20, 20, 20]
    np.testing.assert_array_equal(t, np.concatenate([t1, t1, t1]))


@pytest.mark.parametrize("ms,genes", [([8, 6], [4, 4]), ([0, 4], [4, 4]), ([5], [2])])
def test_pack_raises_on_bad_m(ms, genes):
    with pytest.raises(ValueError):
        P.pack_test_inputs([np.zeros((m, 3)) for m in ms], genes)


def test_pack_raises_on_bad_shapes():
    with pytest.raises(ValueError):
        P.pack_test_inputs([np.zeros((4, 3))], [4, 4])  # one array for two problems
    with pytest.raises(ValueError):
        P.pack_test_inputs([np.zeros((4, 2))], [4])
    with pytest.raises(ValueError):
        P.unpack_outputs([4, 4], np.zeros(7))
    with pytest.raises(ValueError):
        P.unpack_outputs([4, 4], np.zeros(8), None, np.zeros(31))


def test_symbol_is_exported_and_null_ctx_is_rejected():
    lib = _lib.load_library()
    assert hasattr(lib, "lfm_batch_posterior_f64")
    one = np.zeros(4)
    rc = lib.lfm_batch_posterior_f64(None, None, None, None, None, None, None, None, None, None,
                                     None)
    assert rc == _lib.LFM_E_ARG
    m = np.asarray([1], np.int64)
    rc = lib.lfm_batch_posterior_f64(None, None, _lib.dptr(one), None, _lib.dptr(one),
                                     _lib.dptr(m), _lib.dptr(one), _lib.dptr(one),
                                     _lib.dptr(one), None, None)
    assert rc == _lib.LFM_E_ARG


def test_batch_predictor_is_exported():
    import dis_project_amd

    assert dis_project_amd.BatchPredictor is P.BatchPredictor
