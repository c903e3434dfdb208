"""GPU: mi_mcmc_draw_stats_nested and mi_mcmc_draw_stats_nested_ranked -- the nested R-hat of a draws slab [n_keep][d][C] whose chains are K = C / M
superchains of M consecutive chains (draws_nested.hip).

BIT FOR BIT: every output is compared as uint64, any NaN matching any NaN, with mcmc_amd/nested_rhat.py -- the numpy statement of include/mi_mcmc.h's
definition and of every reduction order in it.  No tolerance: a tree taken in another order, a lane holding other elements, a fold not started from
+0.0, a member read twice or a chain given to another superchain changes bits (tests/test_nested_rhat_ref_cpu.py counts how many, and holds the mirror
to exact arithmetic with derived bounds).  tests/draws_nested_cases.py lists the shapes and what each reaches.

END TO END (the last test): hmc on a dense Gaussian, d = 16, K = 64 starting points drawn 10 standard deviations wide, M = 16 chains per point
(nested_rhat.superchain_init), step 0.3, 8 leapfrog steps, seed 5.  The line is sqrt(1 + c / M) with c = 3: for converged superchains
(nrhat^2 - 1) M is chi^2_63 / 63 over within / variance; the first exceeds 2.16 with probability 3e-7 (Wilson-Hilferty at z = 5), the second, with
K (M - 1) = 960 degrees of freedom, is below 0.77 with the same, 2.16 / 0.77 = 2.8 < 3, sixteen dimensions.  The engine is the CPU oracle bit for bit,
and the oracle gives: the starting points themselves nrhat = inf in every dimension (within = 0); after one draw nrhat 10.3 .. 25.9; after a burn-in of
200 draws nrhat 1.014 .. 1.042, (nrhat^2 - 1) M at most 1.38 -- against the line's 1.0897 and 3."""
import functools
import math

import numpy as np
import pytest

import draws_nested_cases as cases
import mcmc_amd
from mcmc_amd import nested_rhat as NR

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _run(shape):
    """ONE all-outputs engine call on the shape's host slab -- shared, read-only"""
    res = mcmc_amd.draw_stats_nested(cases.frozen_slab(shape), shape[3])
    for v in res.values():
        v.setflags(write=False)
    return res


@pytest.mark.parametrize("shape", cases.SHAPES, ids=cases.shape_id)
def test_every_output_is_the_mirror_bit_for_bit(shape):
    N, d, C, M = shape
    got, ref = _run(shape), cases.reference(shape)
    assert got["super_mean"].shape == (C // M, d) and all(got[k].shape == (d,) for k in cases.OUTPUTS[:5])
    cases.assert_is_the_mirror(got, ref, shape)
    assert all(np.isfinite(got[k]).all() for k in cases.OUTPUTS) and (got["nrhat"] > 1.0).all() and (got["within"] > 0.0).all()


@pytest.mark.parametrize("shape", [(17, 3, 195, 3), (2, 3, 390, 130), (1, 129, 260, 130)], ids=cases.shape_id)
def test_bits_do_not_depend_on_the_call(shape):
    import torch
    N, d, C, M = shape
    slab, ref, base = cases.frozen_slab(shape), cases.reference(shape), _run(shape)
    wants = ["want_" + k for k in cases.OUTPUTS]
    for k in cases.OUTPUTS:                                                               # each single output alone
        got = mcmc_amd.draw_stats_nested(slab, M, **{w: w == "want_" + k for w in wants})
        assert all((got[j] is None) == (j != k) for j in cases.OUTPUTS)
        cases.assert_same(got[k], base[k], ("alone", k))
    dev = torch.from_numpy(np.array(slab)).cuda()                                         # the same slab in device memory, the default stream
    torch.cuda.synchronize()
    got = mcmc_amd.draw_stats_nested(dev, M, N, d, C, mem=mcmc_amd.MEM_DEVICE)
    cases.assert_is_the_mirror(got, ref, "device slab, default stream")
    side = torch.cuda.Stream()                                                            # a caller's stream, the slab written on it just before the call
    half = torch.from_numpy(0.5 * np.array(slab)).cuda()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dev2 = half + half                                                                # exact: the same doubles
        got = mcmc_amd.draw_stats_nested(dev2, M, N, d, C, mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream)
        one = mcmc_amd.draw_stats_nested(dev2, M, N, d, C, mem=mcmc_amd.MEM_DEVICE, stream=side.cuda_stream, want_mean=False, want_between=False,
                                         want_within=False, want_mcse_mean=False, want_super_mean=False)
    cases.assert_is_the_mirror(got, ref, "device slab, caller's stream")
    cases.assert_same(one["nrhat"], base["nrhat"], "device slab, caller's stream, nrhat alone")
    assert np.array_equal(dev.cpu().numpy(), slab) and np.array_equal(dev2.cpu().numpy(), slab)      # the slab is read only


def test_the_state_of_a_real_run_is_the_case_n_keep_1():
    import torch
    d, K, M = 3, 8, 40                                                                    # C = 320: two chain tiles
    init = NR.superchain_init(np.random.default_rng(3).standard_normal((d, K)), M).T
    st = mcmc_amd.default_settings(rng_seed_value=9, n_burnin_draws=3, n_keep_draws=2, n_leap_steps=4, step_size=0.4)
    draws, info = mcmc_amd.sample_device("hmc", mcmc_amd.TARGET_GAUSS_ISO, init, st)
    theta = info["theta"]                                                                 # [d][C] in HBM, as mi_chains.theta
    got = mcmc_amd.draw_stats_nested(theta, M, 1, d, K * M, mem=mcmc_amd.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    host = theta.cpu().numpy()
    cases.assert_is_the_mirror(got, NR.nested_ref(host, M), "theta on the device")
    cases.assert_is_the_mirror(mcmc_amd.draw_stats_nested(host, M), NR.nested_ref(host, M), "theta as a [d, C] host array")
    assert np.array_equal(host, draws[-1].cpu().numpy())
    both = mcmc_amd.draw_stats_nested(draws, M, 2, d, K * M, mem=mcmc_amd.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    cases.assert_is_the_mirror(both, NR.nested_ref(draws.cpu().numpy(), M), "the draws of the same run")


def test_non_finite_and_constant_dimensions_are_the_mirrors_and_stay_alone():
    shape = (3, 129, 6, 2)
    slab = np.array(cases.frozen_slab(shape))
    i_nan, i_inf, i_const = 5, 70, 128
    slab[1, i_nan, 3] = np.nan
    slab[2, i_inf, 0] = np.inf
    slab[:, i_const, :] = 2.5
    got, ref, clean = mcmc_amd.draw_stats_nested(slab, 2), NR.nested_ref(slab, 2), _run(shape)
    cases.assert_is_the_mirror(got, ref, "NaN, +inf and a constant dimension")
    assert np.isnan(got["nrhat"][[i_nan, i_inf, i_const]]).all() and got["mean"][i_inf] == np.inf
    assert got["mean"][i_const] == 2.5 and got["between"][i_const] == 0.0 and got["within"][i_const] == 0.0         # 0 / 0
    touched = np.zeros(shape[1], dtype=bool)
    touched[[i_nan, i_inf, i_const]] = True
    for k in cases.OUTPUTS[:5]:
        assert np.isfinite(got[k][~touched]).all()
        assert np.array_equal(cases.bits(got[k])[~touched], cases.bits(clean[k])[~touched]), k
    assert np.array_equal(cases.bits(got["super_mean"])[:, ~touched], cases.bits(clean["super_mean"])[:, ~touched])
    assert np.isnan(got["super_mean"][3 // 2, i_nan]) and np.isfinite(np.delete(got["super_mean"][:, i_nan], 3 // 2)).all()


@functools.lru_cache(maxsize=None)
def _run_ranked(shape):
    res = mcmc_amd.draw_stats_nested_ranked(cases.frozen_slab(shape), shape[3])
    for v in res.values():
        v.setflags(write=False)
    return res


@pytest.mark.parametrize("shape", cases.RANKED_SHAPES, ids=cases.shape_id)
def test_the_ranked_form_is_the_mirror_bit_for_bit(shape):
    N, d, C, M = shape
    got, ref = _run_ranked(shape), cases.ranked_reference(shape)
    cases.assert_is_the_mirror(got, ref, shape, cases.RANKED_OUTPUTS)
    assert np.array_equal(got["nrhat"], np.maximum(got["nrhat_bulk"], got["nrhat_tail"])) and (got["nrhat"] > 1.0).all()
    lib = mcmc_amd.lib()
    try:                                                                                  # one dimension per group
        lib.mi_mcmc_test_set_rank_ws_bytes(lib.mi_mcmc_test_rank_dim_bytes(N, C, 0, 1))
        assert lib.mi_mcmc_test_rank_dims_per_group(N, d, C, 0, 1) == 1
        grouped = mcmc_amd.draw_stats_nested_ranked(cases.frozen_slab(shape), M)
        alone = [mcmc_amd.draw_stats_nested_ranked(cases.frozen_slab(shape), M, **{"want_" + j: j == k for j in cases.RANKED_OUTPUTS}) for k in cases.RANKED_OUTPUTS]
    finally:
        lib.mi_mcmc_test_set_rank_ws_bytes(0)
    cases.assert_is_the_mirror(grouped, ref, (shape, "one dimension per group"), cases.RANKED_OUTPUTS)
    for k, res in zip(cases.RANKED_OUTPUTS, alone):
        assert all((res[j] is None) == (j != k) for j in cases.RANKED_OUTPUTS)
        cases.assert_same(res[k], ref[k], (shape, "alone, one dimension per group", k))


def test_the_ranked_form_on_the_device_and_with_a_nan():
    import torch
    shape = (17, 3, 195, 3)
    N, d, C, M = shape
    dev = torch.from_numpy(np.array(cases.frozen_slab(shape))).cuda()
    got = mcmc_amd.draw_stats_nested_ranked(dev, M, N, d, C, mem=mcmc_amd.MEM_DEVICE, stream=torch.cuda.current_stream().cuda_stream)
    cases.assert_is_the_mirror(got, cases.ranked_reference(shape), "device slab", cases.RANKED_OUTPUTS)
    slab = np.array(cases.frozen_slab(shape))
    slab[4, 1, 77] = np.nan
    slab[0, 2, 5] = np.inf                                                                # +inf has a finite score: the dimension stays finite
    got, ref, clean = mcmc_amd.draw_stats_nested_ranked(slab, M), NR.nested_ranked_ref(slab, M), _run_ranked(shape)
    cases.assert_is_the_mirror(got, ref, "a NaN and a +inf", cases.RANKED_OUTPUTS)
    for k in cases.RANKED_OUTPUTS:
        assert np.isnan(got[k][1]) and np.isfinite(got[k][[0, 2]]).all()
        assert cases.bits(got[k])[0] == cases.bits(clean[k])[0]


def test_superchains_started_far_apart_read_far_above_the_line_and_below_it_after_a_burn_in():
    import orc
    from mcmc_amd import synth
    d, K, M, c = 16, 64, 16, 3.0
    line = math.sqrt(1.0 + c / M)
    prec = synth.dense_gaussian_precision(d)
    sd = np.sqrt(np.diag(np.linalg.inv(prec)))
    theta0 = NR.superchain_init(10.0 * sd[:, None] * np.random.default_rng(11).standard_normal((d, K)), M)
    init = np.ascontiguousarray(theta0.T)
    start = mcmc_amd.draw_stats_nested(theta0, M)["nrhat"]
    assert np.isinf(start).all() and (start > 0).all()                                    # members of a superchain coincide: within = 0
    target = orc.TargetSpec(orc.TARGET_DENSE, d, prec=prec, W=4)
    seen = {}
    for burn in (0, 200):
        st = mcmc_amd.default_settings(rng_seed_value=5, n_burnin_draws=burn, n_keep_draws=1, n_leap_steps=8, step_size=0.3)
        _, info = mcmc_amd.hmc(mcmc_amd.TARGET_GAUSS_DENSE, init, st, prec=prec)
        o_draws, _ = orc.run_many(orc.ALGO_HMC, target, init, orc.make_settings(seed=5, n_burnin=burn, n_keep=1, n_leap=8, step=0.3, W=4))
        assert np.array_equal(info["theta"], o_draws[0])
        got = mcmc_amd.draw_stats_nested(info["theta"], M)
        cases.assert_is_the_mirror(got, NR.nested_ref(o_draws[0], M), f"theta after {burn + 1} draws")
        seen[burn] = got["nrhat"]
        print(f"after {burn + 1} draws: nrhat {seen[burn].min():.4f} .. {seen[burn].max():.4f}, (nrhat^2 - 1) M at most {((seen[burn] ** 2 - 1.0) * M).max():.3f}; "
              f"the line: {line:.4f}")
    assert (seen[0] > 4.0).all()
    assert (seen[200] < line).all() and (seen[200] > 1.0).all()
