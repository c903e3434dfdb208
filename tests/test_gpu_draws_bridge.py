"""GPU: mi_mcmc_bridge_proposal, mi_mcmc_bridge_estimate and mi_mcmc_draws_bridge (mcmc_amd/csrc/draws_bridge.hip) against mcmc_amd/bridge.py run over the
CPU oracle's arithmetic -- orc.dot(x, y, 1) and orc.dot(x, y, 4), orc.math_eval 0 / 1 / 3 (exp / log / softplus), orc.normal_vec on stream 7, the oracle's
inverse and Cholesky.  BIT FOR BIT: every output is compared as uint64 and any NaN matches any NaN; the one tolerance in this file is the end-to-end
run's, the estimator's own ESS-corrected five sigma.

Shapes (n_keep, d, C, n_fit, n_prop), the smallest at which each piece can go wrong:
  DENSE     (2, 1, 3, 0, 0)       below every tile
            (4, 5, 7, 0, 0)
            (5, 17, 37, 2, 50)    a ragged contraction, an odd n_keep, N2 != N1 and no multiple of 16
            (2, 130, 333, 0, 0)   two row tiles, an odd C
            (4, 3, 8200, 0, 0)    N1 = 16 400: two pieces of SUMP, nine chunks of the moments
            (4, 32, 40, 0, 0)     contraction steps that are all full
  LOGISTIC  (4, 3, 37) with 5 rows, (4, 70, 333) with 130 rows;  ISO, DIAG (4, 20, 37)."""
import functools

import numpy as np
import pytest

import mcmc_amd
import orc
from linalg_cases import orc_chol, orc_inv
from mcmc_amd import bridge, ess, synth

pytestmark = pytest.mark.gpu

ORC_MATH = dict(dot=lambda a, b: orc.dot(a, b, 1), dot4=lambda a, b: orc.dot(a, b, 4), exp=lambda x: orc.math_eval(0, x)[0], log=lambda x: orc.math_eval(1, x)[0],
                softplus=lambda x: orc.math_eval(3, x)[0], normal_vec=lambda seed, i, d: orc.normal_vec(seed, i, 0, bridge.STREAM_BRIDGE, d),
                chol_lower=orc_chol, inverse=orc_inv)
SEED = 0x1234567890ABCDEF
DENSE_SHAPES = [(2, 1, 3, 0, 0), (4, 5, 7, 0, 0), (5, 17, 37, 2, 50), (2, 130, 333, 0, 0), (4, 3, 8200, 0, 0), (4, 32, 40, 0, 0)]
LOGIT_SHAPES = [((4, 3, 37, 0, 0), 5), ((4, 70, 333, 0, 0), 130)]
RAGGED = DENSE_SHAPES[2]
_KIND = {"iso": mcmc_amd.TARGET_GAUSS_ISO, "diag": mcmc_amd.TARGET_GAUSS_DIAG, "dense": mcmc_amd.TARGET_GAUSS_DENSE, "logistic": mcmc_amd.TARGET_LOGISTIC}
_ids = lambda s: "x".join(map(str, s)) if isinstance(s, tuple) else f"{s}rows"


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _assert_same(got, want, what):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = ~((np.isnan(got) & np.isnan(want)) | (_bits(got) == _bits(want)))
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:4].tolist(), got[bad][:4].tolist(), want[bad][:4].tolist())


def _summary(res):
    return np.array([res["summary"][k] for k in bridge.SUMMARY])


@functools.lru_cache(maxsize=None)
def _problem(name, d, n_rows=0):
    """(prec, X, y) of a target, read-only"""
    if name == "iso":
        return None, None, None
    if name == "diag":
        out = synth.ill_conditioned_diag(d, 50.0), None, None
    elif name == "dense":
        out = synth.dense_gaussian_precision(d), None, None
    else:
        out = (None,) + synth.logistic_problem(d, n_rows)
    for a in out:
        if a is not None:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _slab(name, shape, n_rows=0):
    """a slab that looks like posterior draws of the target: N(m, V) with V near the posterior's scale, so that the iteration converges in a few steps"""
    n, d, C_ = shape[:3]
    rng = np.random.default_rng(n * 1000003 + d * 1009 + C_)
    x = rng.standard_normal((n, d, C_))
    if name == "dense":
        Lc = np.linalg.cholesky(np.linalg.inv(_problem(name, d)[0]))
        x = np.einsum("ab,tbc->tac", Lc, x)
    elif name == "diag":
        x = x / np.sqrt(_problem(name, d)[0])[None, :, None]
    elif name == "logistic":
        x = 0.7 * x + 0.3
    x = np.ascontiguousarray(x)
    x.setflags(write=False)
    return x


def _target(name, d, n_rows=0):
    prec, X, y = _problem(name, d, n_rows)
    return mcmc_amd.make_target(_KIND[name], d, prec=prec, X=X, y=y)


@functools.lru_cache(maxsize=None)
def _reference(name, shape, n_rows=0, max_iter=0):
    n, d, C_, n_fit, n_prop = shape
    prec, X, y = _problem(name, d, n_rows)
    return bridge.bridge_ref(_KIND[name], _slab(name, shape, n_rows), prec=prec, X=X, y=y, n_fit=n_fit, n_prop=n_prop, seed=SEED, max_iter=max_iter, math=ORC_MATH)


def _assert_bridge(res, ref, what):
    _assert_same(_summary(res), ref["summary"], (what, "summary"))
    for k in ("f2", "mean", "cov"):
        if res[k] is not None:
            _assert_same(res[k], ref[k], (what, k))


def _check_case(name, shape, n_rows=0):
    n, d, C_, n_fit, n_prop = shape
    ref = _reference(name, shape, n_rows)
    slab = _slab(name, shape, n_rows)
    # the proposal first: what a failure of the whole would come from
    p = mcmc_amd.bridge_proposal(slab, n_fit=n_fit, n_prop=n_prop, seed=SEED)
    rp = ref["proposal"]
    assert p["status"] == rp["status"] == 0
    _assert_same(p["mean"], rp["mean"], (shape, "mean"))
    _assert_same(p["cov"], rp["cov"], (shape, "cov"))
    _assert_same(np.float64(p["ldh"]), np.float64(rp["ldh"]), (shape, "ldh"))
    _assert_same(p["prop"], rp["prop"], (shape, "prop"))
    _assert_same(p["logg_post"], rp["logg_post"], (shape, "logg_post"))
    _assert_same(p["logg_prop"], rp["logg_prop"], (shape, "logg_prop"))
    res = mcmc_amd.draws_bridge(_target(name, d, n_rows), slab, n_fit=n_fit, n_prop=n_prop, seed=SEED)
    _assert_bridge(res, ref, shape)
    assert res["summary"]["status"] in (0, 2) and np.isfinite(res["summary"]["logml"])
    assert "bridge_propose_kernel" in mcmc_amd.last_kernel() and "bridge_pieces_kernel" in mcmc_amd.last_kernel()
    return res, ref


@pytest.mark.parametrize("shape", DENSE_SHAPES, ids=_ids)
def test_dense_is_the_mirror_bit_for_bit(shape):
    res, ref = _check_case("dense", shape)
    n, d, C_ = shape[:3]
    if d == 3:                                           # the analytic value, within the estimator's own five sigma (i.i.d. draws)
        truth = 0.5 * d * bridge.LOG_2PI - 0.5 * np.linalg.slogdet(_problem("dense", d)[0])[1]
        assert abs(res["summary"]["logml"] - truth) <= 5.0 * np.sqrt(res["summary"]["cv1"] + res["summary"]["cv2"])


@pytest.mark.parametrize("shape,n_rows", LOGIT_SHAPES, ids=_ids)
def test_logistic_is_the_mirror_bit_for_bit(shape, n_rows):
    _check_case("logistic", shape, n_rows)


@pytest.mark.parametrize("name", ["iso", "diag"])
def test_separable_gaussians_are_the_mirror_bit_for_bit(name):
    _check_case(name, (4, 20, 37, 0, 0))


def test_a_singular_fit_is_status_one_and_all_nan():
    shape = (4, 17, 3, 0, 0)                             # K0 = 6 <= d
    slab = _slab("dense", shape)
    ref = bridge.bridge_ref(bridge.DENSE, slab, prec=_problem("dense", 17)[0], seed=SEED, math=ORC_MATH)
    assert ref["summary"][1] == 1
    res = mcmc_amd.draws_bridge(_target("dense", 17), slab, seed=SEED)            # (returns: the rc is MI_OK)
    _assert_bridge(res, ref, "singular")
    assert res["summary"]["status"] == 1 and np.isnan(res["f2"]).all() and np.isnan(res["mean"]).all() and np.isnan(res["cov"]).all()
    assert np.isnan(_summary(res)[[0, 2, 3, 4, 5, 6]]).all() and res["summary"]["n_prop"] == 6
    p = mcmc_amd.bridge_proposal(slab, seed=SEED)
    assert p["status"] == 1 and np.isnan(p["ldh"])
    for k in ("prop", "logg_post", "logg_prop", "mean", "cov"):
        assert np.isnan(p[k]).all(), k


def test_a_nan_in_the_fit_part_is_status_one():
    slab = np.array(_slab("dense", (4, 5, 7, 0, 0)))
    slab[1, 2, 3] = np.nan
    res = mcmc_amd.draws_bridge(_target("dense", 5), slab, seed=SEED)
    assert res["summary"]["status"] == 1 and np.isnan(res["summary"]["logml"]) and np.isnan(res["f2"]).all()
    ref = bridge.bridge_ref(bridge.DENSE, slab, prec=_problem("dense", 5)[0], seed=SEED, math=ORC_MATH)
    _assert_bridge(res, ref, "nan in the fit part")


def test_an_inf_in_the_iteration_part_alone_is_status_three_as_the_mirror_gives():
    slab = np.array(_slab("dense", (4, 5, 7, 0, 0)))
    slab[3, 2, 3] = np.inf
    res = mcmc_amd.draws_bridge(_target("dense", 5), slab, seed=SEED)
    ref = bridge.bridge_ref(bridge.DENSE, slab, prec=_problem("dense", 5)[0], seed=SEED, math=ORC_MATH)
    _assert_bridge(res, ref, "inf in the iteration part")
    assert res["summary"]["status"] == 3 and np.isnan(res["summary"]["logml"])


def test_max_iter_one_is_status_two_with_the_mirrors_r():
    shape = DENSE_SHAPES[1]
    ref = _reference("dense", shape, 0, 1)
    res = mcmc_amd.draws_bridge(_target("dense", shape[1]), _slab("dense", shape), seed=SEED, max_iter=1)
    _assert_bridge(res, ref, "max_iter = 1")
    assert res["summary"]["status"] == 2 and res["summary"]["it"] == 1 and np.isfinite(res["summary"]["logml"])


@pytest.mark.parametrize("name,shape,n_rows", [("dense", RAGGED, 0), ("logistic", LOGIT_SHAPES[0][0], 5)], ids=["dense", "logistic"])
def test_the_three_calls_by_hand_are_draws_bridge(name, shape, n_rows):
    n, d, C_, n_fit, n_prop = shape
    slab, tgt = _slab(name, shape, n_rows), _target(name, d, n_rows)
    whole = mcmc_amd.draws_bridge(tgt, slab, n_fit=n_fit, n_prop=n_prop, seed=SEED)
    p = mcmc_amd.bridge_proposal(slab, n_fit=n_fit, n_prop=n_prop, seed=SEED)
    nf = n_fit or n // 2
    lp1 = mcmc_amd.draws_log_kernel(tgt, slab[nf:])
    lp2 = mcmc_amd.draws_log_kernel(tgt, p["prop"])[0]
    e = mcmc_amd.bridge_estimate(lp1, p["logg_post"], lp2, p["logg_prop"])
    _assert_same(_summary(e), _summary(whole), "summary")
    _assert_same(e["f2"], whole["f2"], "f2")
    _assert_same(p["mean"], whole["mean"], "mean")
    _assert_same(p["cov"], whole["cov"], "cov")
    ref = _reference(name, shape, n_rows)
    _assert_same(lp1, ref["logp_post"], "logp_post")
    _assert_same(lp2, ref["logp_prop"], "logp_prop")


def test_a_device_slab_equals_the_host_slab():
    import torch
    n, d, C_, n_fit, n_prop = RAGGED
    ref = _reference("dense", RAGGED)
    slab = _slab("dense", RAGGED)
    dev = torch.from_numpy(np.array(slab)).cuda()
    st = torch.cuda.current_stream().cuda_stream
    n_it, N2 = n - n_fit, n_prop
    f2 = torch.full((n_it, C_), -7.0, dtype=torch.float64, device="cuda")
    res = mcmc_amd.draws_bridge(_target("dense", d), dev, n_fit=n_fit, n_prop=n_prop, seed=SEED, n_keep=n, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, f2=f2)
    res["f2"] = f2.cpu().numpy()
    _assert_bridge(res, ref, "device slab")
    outs = dict(prop=torch.full((1, d, N2), -7.0, dtype=torch.float64, device="cuda"), logg_post=torch.full((n_it, C_), -7.0, dtype=torch.float64, device="cuda"),
                logg_prop=torch.full((N2,), -7.0, dtype=torch.float64, device="cuda"))
    p = mcmc_amd.bridge_proposal(dev, n_fit=n_fit, n_prop=n_prop, seed=SEED, n_keep=n, d=d, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, **outs)
    for k, v in outs.items():
        _assert_same(v.cpu().numpy(), ref["proposal"][k], ("device slab", k))
    # the estimate from device arrays; without prop_out the proposal runs in groups: the same logg_prop
    lp1 = torch.from_numpy(ref["logp_post"]).cuda()
    lp2 = torch.from_numpy(ref["logp_prop"]).cuda()
    f2.fill_(-7.0)
    e = mcmc_amd.bridge_estimate(lp1, outs["logg_post"], lp2, outs["logg_prop"], n_it=n_it, n_chains=C_, n_prop=N2, mem=mcmc_amd.MEM_DEVICE, stream=st, f2=f2)
    _assert_same(_summary(e), ref["summary"], "device estimate")
    _assert_same(f2.cpu().numpy(), ref["f2"], "device estimate f2")
    lg2 = torch.full((N2,), -7.0, dtype=torch.float64, device="cuda")
    mcmc_amd.bridge_proposal(dev, n_fit=n_fit, n_prop=n_prop, seed=SEED, n_keep=n, d=d, n_chains=C_, mem=mcmc_amd.MEM_DEVICE, stream=st, logg_prop=lg2)
    _assert_same(lg2.cpu().numpy(), ref["proposal"]["logg_prop"], "logg_prop alone")
    assert np.array_equal(dev.cpu().numpy(), slab)       # the slab is read only


def test_the_proposal_group_budget_does_not_change_a_bit():
    n, d, C_, n_fit, n_prop = RAGGED                                   # 50 proposal columns in groups of 16: 16 + 16 + 16 + 2
    ref = _reference("dense", RAGGED)
    slab = _slab("dense", RAGGED)
    mcmc_amd.test_set_bridge_prop_bytes(16 * d * 8)
    try:
        res = mcmc_amd.draws_bridge(_target("dense", d), slab, n_fit=n_fit, n_prop=n_prop, seed=SEED)
        p = mcmc_amd.bridge_proposal(slab, n_fit=n_fit, n_prop=n_prop, seed=SEED, want_prop=False)
        mcmc_amd.test_set_bridge_prop_bytes(128 * d * 8)               # 300 columns in groups of 128: 128 + 128 + 44
        q = mcmc_amd.bridge_proposal(slab, n_fit=n_fit, n_prop=300, seed=SEED, want_prop=False)
    finally:
        mcmc_amd.test_set_bridge_prop_bytes(0)
    _assert_bridge(res, ref, "four groups")
    _assert_same(p["logg_prop"], ref["proposal"]["logg_prop"], "four groups, logg_prop")
    whole = mcmc_amd.bridge_proposal(slab, n_fit=n_fit, n_prop=300, seed=SEED)
    _assert_same(q["logg_prop"], whole["logg_prop"], "three groups of 128, logg_prop")
    _assert_same(whole["logg_prop"][:50], ref["proposal"]["logg_prop"], "a proposal column does not depend on how many follow")


def test_a_grid_cap_does_not_change_a_bit():
    shape = DENSE_SHAPES[4]
    ref = _reference("dense", shape)
    mcmc_amd.test_set_grid_cap(2)
    try:
        res = mcmc_amd.draws_bridge(_target("dense", shape[1]), _slab("dense", shape), seed=SEED)
    finally:
        mcmc_amd.test_set_grid_cap(0)
    _assert_bridge(res, ref, "grid cap 2")


def test_two_calls_give_the_same_bits():
    shape, n_rows = LOGIT_SHAPES[1]
    tgt, slab = _target("logistic", shape[1], n_rows), _slab("logistic", shape, n_rows)
    a = mcmc_amd.draws_bridge(tgt, slab, seed=SEED)
    mcmc_amd.release_workspace()
    b = mcmc_amd.draws_bridge(tgt, slab, seed=SEED)
    _assert_same(_summary(a), _summary(b), "summary")
    _assert_same(a["f2"], b["f2"], "f2")
    c = mcmc_amd.draws_bridge(tgt, slab, seed=SEED + 1)
    assert c["summary"]["logml"] != a["summary"]["logml"]              # ... and the seed is read


def test_targets_without_the_whole_space_as_support_are_refused():
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_bridge(mcmc_amd.make_target(mcmc_amd.TARGET_NORMAL_MODEL, 2, y=np.ones(5)), np.ones((4, 2, 5)))
    assert e.value.code == mcmc_amd.MI_ERR_UNSUPPORTED
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draws_bridge(mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_MIXTURE, 2), np.ones((4, 2, 5)))
    assert e.value.code == mcmc_amd.MI_ERR_UNSUPPORTED


def test_end_to_end_hmc_on_a_dense_gaussian_meets_the_analytic_value():
    d, C_, n_keep = 16, 1024, 8
    P = synth.dense_gaussian_precision(d)
    st = mcmc_amd.default_settings(n_burnin_draws=200, n_keep_draws=n_keep, n_leap_steps=8, step_size=0.2, rng_seed_value=7)
    draws, _ = mcmc_amd.sample("hmc", mcmc_amd.TARGET_GAUSS_DENSE, synth.initial_states(C_, d), st, prec=P)
    res = mcmc_amd.draws_bridge(mcmc_amd.make_target(mcmc_amd.TARGET_GAUSS_DENSE, d, prec=P), draws, seed=SEED)
    truth = 0.5 * d * bridge.LOG_2PI - 0.5 * np.linalg.slogdet(P)[1]
    n_it = n_keep - n_keep // 2
    e = ess.ess_per_chain(res["f2"][:, None, :])[0]
    err, bound = abs(res["summary"]["logml"] - truth), 5.0 * np.sqrt(bridge.rel_mse(_summary(res), n_it, e))
    print(f"end to end d=16: logml {res['summary']['logml']:.6f} truth {truth:.6f} error {err:.3e} bound {bound:.3e} ESS per chain {e:.2f} of {n_it} it {int(res['summary']['it'])}")
    assert res["summary"]["status"] == 0
    assert err <= bound
