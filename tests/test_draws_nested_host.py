"""No GPU: mi_mcmc_draw_stats_nested and mi_mcmc_draw_stats_nested_ranked reject bad arguments before any device call (MI_ERR_BAD_ARG even where no
device is visible -- a call that reached the device probe would answer MI_ERR_NO_DEVICE there)."""

import numpy as np
import pytest

import mcmc_amd

# N = 2, d = 3, C = 8, M = 2 is a good call; every case changes what makes it a bad one
CASES = {
    "null_slab": (dict(slab=None), "null slab"),
    "all_outputs_null": (dict(outs=0), "outputs are NULL"),
    "d_is_0": (dict(d=0), "d must be positive"),
    "d_beyond_65536": (dict(d=65537), "is beyond 65536"),
    "n_keep_is_0": (dict(n_keep=0), "must be positive"),
    "n_chains_is_0": (dict(n_chains=0), "must be positive"),
    "n_keep_beyond_32_bits": (dict(n_keep=1 << 32), "do not fit 32 bits"),
    "n_chains_beyond_32_bits": (dict(n_chains=1 << 32, M=1 << 16), "do not fit 32 bits"),
    "M_is_0": (dict(M=0), "chains_per_super must be positive"),
    "M_does_not_divide_C": (dict(M=3), "not a multiple"),
    "K_is_1": (dict(M=8), "at least 2 superchains"),
    "M_beyond_C": (dict(M=16), "not a multiple"),
    "N_is_1_with_M_is_1": (dict(n_keep=1, M=1), "identically 0"),
}


def _call(ranked, slab=True, outs=None, n_keep=2, d=3, n_chains=8, M=2):
    x = np.zeros((2, 3, 8))
    n_out = 3 if ranked else 6
    bufs = [np.zeros(64) for _ in range(n_out)]
    ptrs = [b.ctypes.data for b in bufs] if outs is None else [None] * n_out
    fn = mcmc_amd.lib().mi_mcmc_draw_stats_nested_ranked if ranked else mcmc_amd.lib().mi_mcmc_draw_stats_nested
    return fn(x.ctypes.data if slab else None, mcmc_amd.MEM_HOST, n_keep, d, n_chains, M, *ptrs, None)


@pytest.mark.parametrize("ranked", [False, True], ids=["nested", "nested_ranked"])
@pytest.mark.parametrize("case", list(CASES))
def test_bad_arguments_are_rejected_without_a_gpu(case, ranked):
    kw, text = CASES[case]
    assert _call(ranked, **kw) == mcmc_amd.MI_ERR_BAD_ARG
    msg = mcmc_amd.lib().mi_mcmc_last_error().decode()
    assert msg.startswith("draw_stats_nested_ranked: " if ranked else "draw_stats_nested: "), msg
    assert text in msg, msg


def test_the_ranked_form_also_needs_fewer_than_2_to_the_32_samples():
    assert _call(True, n_keep=1 << 16, n_chains=1 << 16, M=2) == mcmc_amd.MI_ERR_BAD_ARG
    assert b"draw_stats_nested_ranked" in mcmc_amd.lib().mi_mcmc_last_error()


def test_every_single_output_is_enough_for_the_checks():
    """one output alone passes validation: the call goes on to the device probe (MI_OK with a device, MI_ERR_NO_DEVICE without), never BAD_ARG"""
    x = np.random.default_rng(0).standard_normal((2, 3, 8))
    for ranked, n_out in ((False, 6), (True, 3)):
        fn = mcmc_amd.lib().mi_mcmc_draw_stats_nested_ranked if ranked else mcmc_amd.lib().mi_mcmc_draw_stats_nested
        for a in range(n_out):
            buf = np.zeros(64)
            ptrs = [buf.ctypes.data if b == a else None for b in range(n_out)]
            assert fn(x.ctypes.data, mcmc_amd.MEM_HOST, 2, 3, 8, 2, *ptrs, None) in (mcmc_amd.MI_OK, mcmc_amd.MI_ERR_NO_DEVICE)


def test_front_ends_raise():
    for fn in (mcmc_amd.draw_stats_nested, mcmc_amd.draw_stats_nested_ranked):
        with pytest.raises(mcmc_amd.MiMcmcError) as e:
            fn(np.zeros((2, 3, 8)), 3)
        assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG and "draw_stats_nested" in str(e.value)
        with pytest.raises(mcmc_amd.MiMcmcError) as e:
            fn(np.zeros((3, 8)), 1)                                     # a state [d, C] is n_keep = 1, and M = 1 leaves nothing within
        assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
        with pytest.raises(mcmc_amd.MiMcmcError) as e:
            fn(np.zeros((3, 8)), 0)
        assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draw_stats_nested(np.zeros((2, 3, 8)), 2, want_nrhat=False, want_mean=False, want_between=False, want_within=False, want_mcse_mean=False,
                                   want_super_mean=False)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG
    with pytest.raises(mcmc_amd.MiMcmcError) as e:
        mcmc_amd.draw_stats_nested_ranked(np.zeros((2, 3, 8)), 2, want_nrhat=False, want_nrhat_bulk=False, want_nrhat_tail=False)
    assert e.value.code == mcmc_amd.MI_ERR_BAD_ARG


def test_new_entry_points_are_exported():
    for name in ("mi_mcmc_draw_stats_nested", "mi_mcmc_draw_stats_nested_ranked"):
        assert name in mcmc_amd.EXPORTS and hasattr(mcmc_amd.lib(), name)
    assert mcmc_amd.lib().mi_mcmc_version() == 0x000600
