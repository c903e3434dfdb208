"""GPU: mi_mcmc_draws_predict -- p[r][k] = sigmoid(X_r . x_k) of every row of the target's X at every column of a slab [n_keep][d][C], the Bernoulli
replicates yrep[r][k] from the counter-based generator, and both folds of the two (mcmc_amd/csrc/draws_predict.hip) against mcmc_amd/predict.py, the numpy
statement of include/mi_mcmc.h's definition, run over the CPU oracle's arithmetic (orc.dot(x, y, 1): the fma chain; orc.math_eval 0 / 1 / 3 / 4: exp /
log / softplus / sigmoid; orc.philox: the raw block).  BIT FOR BIT: every output is compared as uint64 and any NaN matches any NaN.  The one tolerance in
this file, 1e-12 relative, is between two fold orders of the same integers in the end-to-end test (each fold is exact; the two divisions by K differ).

The row kernel's workgroup owns a 128-row tile and a chunk of 2048 columns; the column kernel's 128 columns and all row tiles.  Which shape
(n_keep, d, C) x rows reaches what:
  (2, 3, 5), 5 rows       K = 10, below every tile
  (3, 70, 37), 130 rows   two row tiles, the second with 2 rows; a ragged contraction; a column tile that spans t; an odd C
  (1, 520, 19), 70 rows   33 contraction steps
  (3, 5, 1366), 9 rows    K = 4098 = 2 * 2048 + 2: three chunks, the last with two columns
  (2, 32, 5), 16 rows     d a multiple of 16: a contraction of full steps only
  (2, 4, 200), 260 rows   three row tiles for the column kernel, 400 columns = four column tiles"""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from mcmc_amd import predict, synth

pytestmark = pytest.mark.gpu

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0], sigmoid=lambda x: orc.math_eval(4, x)[0],
                philox=lambda ctr, key: np.array([orc.philox(c, key) for c in ctr], dtype=np.uint32).reshape(-1, 4))
CASES = [((2, 3, 5), 5), ((3, 70, 37), 130), ((1, 520, 19), 70), ((3, 5, 1366), 9), ((2, 32, 5), 16), ((2, 4, 200), 260)]
_IDS = [f"{'x'.join(map(str, s))}-{r}rows" for s, r in CASES]
ROWS_OUT = ("p_mean", "p_var", "rep_freq", "prob", "yrep")          # the row kernel's
COLS_OUT = ("t_rep", "ll_rep", "ll_obs", "summary")                 # the column kernel's
NAMES = ROWS_OUT + COLS_OUT
SEED = 20240611


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((np.isnan(got) & np.isnan(want)) | (_bits(got) == _bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _frozen(*arrays):
    for a in arrays:
        if a is not None:
            a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def _slab(shape):
    rng = np.random.default_rng(shape[0] * 1000003 + shape[1] * 1009 + shape[2])
    return _frozen(rng.standard_normal(shape))[0]


@functools.lru_cache(maxsize=None)
def _problem(d, n_rows):
    return _frozen(*synth.logistic_problem(d, n_rows))


def _target(d, n_rows, with_y=True):
    X, y = _problem(d, n_rows)
    return mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X, y=y if with_y else None)


def _mirror(slab, n_rows, seed=SEED, with_y=True):
    X, y = _problem(slab.shape[1], n_rows)
    return predict.predict_ref(slab, X, y if with_y else None, seed=seed, math=ORC_MATH)


@functools.lru_cache(maxsize=None)
def _reference(shape, n_rows):
    ref = _mirror(_slab(shape), n_rows)
    _frozen(*ref.values())
    return ref


def _summary(res):
    return np.array([res["summary"][k] for k in ("t_obs", "ppp_t", "ppp_dev", "t_rep_mean")])


def _assert_result(res, ref, what):
    for k in NAMES:
        if res[k] is None:
            continue
        _assert_same(_summary(res) if k == "summary" else res[k], ref[k], (what, k))


def _all(target, slab, **kw):
    return mcmc_amd.draws_predict(target, slab, seed=kw.pop("seed", SEED), want_prob=True, want_yrep=True, **kw)


@pytest.mark.parametrize("shape,n_rows", CASES, ids=_IDS)
def test_every_output_is_the_mirror_bit_for_bit(shape, n_rows):
    res = _all(_target(shape[1], n_rows), _slab(shape))
    ref = _reference(shape, n_rows)
    assert all(res[k] is not None for k in NAMES)
    assert res["prob"].shape == res["yrep"].shape == (n_rows, shape[0], shape[2]) and res["t_rep"].shape == (shape[0], shape[2])
    _assert_result(res, ref, shape)
    assert np.isfinite(res["prob"]).all() and ((res["prob"] > 0.0) & (res["prob"] < 1.0)).all() and (res["p_var"] > 0.0).all()
    assert set(np.unique(res["yrep"])) <= {0.0, 1.0}


@pytest.mark.parametrize("shape,n_rows", [CASES[1], CASES[3]], ids=[_IDS[1], _IDS[3]])
def test_every_single_output_alone_gives_the_bits_of_the_full_call(shape, n_rows):
    """each request launches only the kernel it needs (last_kernel says which) and gives the bits of the call that asks for everything"""
    ref = _reference(shape, n_rows)
    tgt, slab = _target(shape[1], n_rows), _slab(shape)
    for k in NAMES:
        res = mcmc_amd.draws_predict(tgt, slab, seed=SEED, **{f"want_{j}": j == k for j in NAMES})
        assert [j for j in NAMES if res[j] is not None] == [k]
        _assert_result(res, ref, ("only", k))
        assert mcmc_amd.last_kernel() == ("predict_rows_kernel" if k in ROWS_OUT else "predict_cols_kernel"), (k, mcmc_amd.last_kernel())
    _all(tgt, slab)
    assert mcmc_amd.last_kernel() == "predict_rows_kernel, predict_cols_kernel"


def _sum4(a):
    q = [0.0, 0.0, 0.0, 0.0]
    for i, v in enumerate(a):
        q[i % 4] = q[i % 4] + float(v)
    return (q[0] + q[2]) + (q[1] + q[3])


@pytest.mark.parametrize("shape,n_rows", [CASES[1], CASES[3], CASES[5]], ids=[_IDS[1], _IDS[3], _IDS[5]])
def test_the_two_kernels_form_the_same_replicates(shape, n_rows):
    """without the mirror: the column kernel's count of a column is the sum of the row kernel's replicates of it, and a row's frequency is the sum of
    its replicates over K -- the quotient is compared as it is formed, A / K (times K it need not round back to the integer)"""
    K = shape[0] * shape[2]
    res = _all(_target(shape[1], n_rows), _slab(shape))
    assert np.array_equal(res["t_rep"], res["yrep"].sum(axis=0))
    assert np.array_equal(_bits(res["rep_freq"]), _bits(res["yrep"].reshape(n_rows, K).sum(axis=1) / np.float64(K)))
    assert np.array_equal(np.rint(res["rep_freq"] * K), res["yrep"].reshape(n_rows, K).sum(axis=1))
    assert res["summary"]["t_rep_mean"] == float(int(res["yrep"].sum())) / float(K)


@pytest.mark.parametrize("shape,n_rows", [CASES[1], CASES[2]], ids=[_IDS[1], _IDS[2]])
def test_ll_obs_is_the_row_sum_of_the_waic_reducers_loglik(shape, n_rows):
    tgt, slab = _target(shape[1], n_rows), _slab(shape)
    ll = mcmc_amd.draws_waic(tgt, slab, want_lppd=False, want_p_waic=False, want_loglik=True, want_summary=False)["loglik"]
    got = mcmc_amd.draws_predict(tgt, slab, seed=SEED, **{f"want_{j}": j == "ll_obs" for j in NAMES})["ll_obs"]
    want = np.array([[_sum4(ll[:, t, c]) for c in range(shape[2])] for t in range(shape[0])])
    _assert_same(got, want, shape)


def test_a_row_of_prob_is_a_slab_the_quantiles_take():
    shape, n_rows = CASES[1]
    res = mcmc_amd.draws_predict(_target(shape[1], n_rows), _slab(shape), seed=SEED, want_prob=True)
    for r in (0, 77, 129):
        row = res["prob"][r].reshape(shape[0], 1, shape[2])                    # [n_keep][1][C]: as it is
        q = mcmc_amd.draws_quantiles(row, [0.05, 0.5, 0.95])
        assert q.shape == (3, 1) and q[0, 0] <= q[1, 0] <= q[2, 0]
        assert res["p_var"][r] > 0.0 and q[0, 0] <= res["p_mean"][r] <= q[2, 0], (r, q.ravel(), res["p_mean"][r])


def test_the_seed_moves_the_replicates_and_nothing_else():
    shape, n_rows = CASES[1]
    ref = _reference(shape, n_rows)
    res = _all(_target(shape[1], n_rows), _slab(shape), seed=SEED + 1)
    assert not np.array_equal(res["yrep"], ref["yrep"]) and not np.array_equal(res["t_rep"], ref["t_rep"])
    for k in ("prob", "p_mean", "p_var", "ll_obs"):
        _assert_same(res[k], ref[k], ("another seed", k))
    assert res["summary"]["t_obs"] == ref["summary"][0]
    # a seed beyond 32 bits reaches the key's second word: the mirror again
    big = (5 << 32) | 77
    res = mcmc_amd.draws_predict(_target(shape[1], n_rows), _slab(shape), seed=big, want_yrep=True, want_t_rep=False, want_ll_rep=False, want_ll_obs=False,
                                 want_summary=False, want_p_mean=False, want_p_var=False, want_rep_freq=False)
    X, _ = _problem(shape[1], n_rows)
    K = shape[0] * shape[2]
    want = predict.yrep(ref["prob"], predict.uniforms(big, n_rows, K, ORC_MATH))
    _assert_same(res["yrep"], want, "a 64-bit seed")


def test_a_target_without_outcomes_gives_the_same_bits():
    shape, n_rows = CASES[1]
    ref = _reference(shape, n_rows)
    res = _all(_target(shape[1], n_rows, with_y=False), _slab(shape))
    assert res["ll_obs"] is None and res["summary"] is None
    for k in ("p_mean", "p_var", "rep_freq", "t_rep", "ll_rep", "prob", "yrep"):
        _assert_same(res[k], ref[k], ("y = None", k))
    cols_only = mcmc_amd.draws_predict(_target(shape[1], n_rows, with_y=False), _slab(shape), seed=SEED, want_p_mean=False, want_p_var=False, want_rep_freq=False)
    _assert_same(cols_only["t_rep"], ref["t_rep"], "y = None, the column kernel alone")
    _assert_same(cols_only["ll_rep"], ref["ll_rep"], "y = None, the column kernel alone")


def test_non_finite_draws_propagate_and_stay_in_their_own_column():
    shape, n_rows = CASES[1]
    n, d, C_ = shape
    x = np.array(_slab(shape))
    x[1, 7, 5] = np.nan
    x[n - 1, 3, 20] = np.inf
    touched = np.zeros((n, C_), dtype=bool)
    touched[1, 5] = touched[n - 1, 20] = True
    res = _all(_target(d, n_rows), x)
    ref = _mirror(x, n_rows)
    clean = _reference(shape, n_rows)
    _assert_result(res, ref, "the touched columns included")                  # prob, t_rep, ll_rep, ll_obs of the two columns and the rows' statistics
    assert np.isnan(ref["prob"][:, 1, 5]).all() and (ref["yrep"][:, 1, 5] == 0.0).all() and ref["t_rep"][1, 5] == 0.0 and np.isnan(ref["ll_rep"][1, 5])
    assert not np.isfinite(ref["ll_obs"][n - 1, 20]) and set(np.unique(ref["prob"][:, n - 1, 20])) <= {0.0, 1.0}      # X_r3 = 0 would give NaN: none is
    for k in ("prob", "yrep"):
        assert np.array_equal(_bits(res[k])[:, ~touched], _bits(clean[k])[:, ~touched]), k
    for k in ("t_rep", "ll_rep", "ll_obs"):
        assert np.array_equal(_bits(res[k])[~touched], _bits(clean[k])[~touched]), k
    assert np.isnan(res["p_mean"]).all() and np.isnan(res["p_var"]).all()         # a NaN among a row's K values: by the IEEE rules, nothing is filtered
    assert np.isfinite(res["rep_freq"]).all()                                     # its replicate is a 0


def test_a_device_slab_with_a_device_target_gives_the_bits_of_the_host_call():
    import torch
    shape, n_rows = CASES[3]                                                      # three chunks: the counting kernel has 17 workgroups to cap
    n, d, C_ = shape
    ref = _reference(shape, n_rows)
    X, y = _problem(d, n_rows)
    dev = torch.from_numpy(np.array(_slab(shape))).cuda()
    X_dev, y_dev = torch.from_numpy(np.array(X)).cuda(), torch.from_numpy(np.array(y)).cuda()
    tgt = mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, d, X=X_dev, y=y_dev, mem=mcmc_amd.MEM_DEVICE)
    assert int(tgt.n_rows) == n_rows

    def outs():
        f = lambda *s: torch.full(s, -7.0, dtype=torch.float64, device="cuda")
        return dict(p_mean=f(n_rows), p_var=f(n_rows), rep_freq=f(n_rows), prob=f(n_rows, n, C_), yrep=f(n_rows, n, C_), t_rep=f(n, C_), ll_rep=f(n, C_), ll_obs=f(n, C_))

    def run(stream, want_summary, o):
        return mcmc_amd.draws_predict(tgt, dev, seed=SEED, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=stream.cuda_stream, want_summary=want_summary, **o)

    torch.cuda.synchronize()
    s1 = torch.cuda.Stream()
    # enqueued only: two calls in a row on one stream, the second into its own outputs; nothing is read before the stream has been waited for
    a, b = outs(), outs()
    ra = run(s1, False, a)
    rb = run(s1, False, b)
    assert ra["summary"] is None and rb["summary"] is None
    s1.synchronize()
    for o, what in ((a, "first enqueued call"), (b, "second enqueued call")):
        got = {k: v.cpu().numpy() for k, v in o.items()}
        got["summary"] = None
        _assert_result(got, ref, what)
    # with the summary the call blocks; a lowered grid cap changes no bit (the pack and counting kernels make several passes)
    mcmc_amd.test_set_grid_cap(2)
    try:
        c = outs()
        rc = run(torch.cuda.current_stream(), True, c)
    finally:
        mcmc_amd.test_set_grid_cap(0)
    torch.cuda.synchronize()
    got = {k: v.cpu().numpy() for k, v in c.items()}
    got["summary"] = rc["summary"]
    _assert_result(got, ref, "device slab, summary, grid cap 2")
    assert np.array_equal(dev.cpu().numpy(), _slab(shape))                        # the slab is read only


def test_end_to_end_on_sampled_draws():
    X, y = synth.logistic_problem(4, 60)
    st = mcmc_amd.default_settings(rng_seed_value=5, n_burnin_draws=40, n_keep_draws=8, n_leap_steps=8, step_size=0.1)
    draws, _ = mcmc_amd.sample("hmc", mcmc_amd.TARGET_LOGISTIC, 0.1 * synth.initial_states(256, 4, seed=8), st, X=X, y=y)
    assert draws.shape == (8, 4, 256)
    res = mcmc_amd.draws_predict(mcmc_amd.make_target(mcmc_amd.TARGET_LOGISTIC, 4, X=X, y=y), draws, seed=1, want_prob=True, want_yrep=True)
    for k in NAMES[:-1]:
        assert np.isfinite(res[k]).all(), k
    s = res["summary"]
    assert all(np.isfinite(v) for v in s.values()) and s["t_obs"] == y.sum()
    assert 0.0 <= s["ppp_t"] <= 1.0 and 0.0 <= s["ppp_dev"] <= 1.0
    assert abs(s["t_rep_mean"] - res["rep_freq"].sum()) <= 1e-12 * abs(s["t_rep_mean"]), (s["t_rep_mean"], res["rep_freq"].sum())
    print(f"t_obs = {s['t_obs']}, t_rep_mean = {s['t_rep_mean']:.3f}, ppp_t = {s['ppp_t']:.3f}, ppp_dev = {s['ppp_dev']:.3f}")
