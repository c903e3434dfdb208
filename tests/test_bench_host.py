"""CPU: the host logic of bench.py that needs no GPU -- which committed profile a traffic figure may be quoted from, and that an N-GPU
line is refused when the devices are not there."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def test_traffic_is_only_quoted_from_a_profile_of_the_kernel_that_ran():
    """profiles/ lookup: newest round first, and only a PMC pass of this workload AND of the kernel mi_mcmc_last_kernel named."""
    import bench
    key = (4, 65536, 128, 200)
    t, src = bench.profiled_traffic(4, key, "nuts_gauss_dyn_kernel<8, false>")
    assert t is not None and src.startswith("profiles/r") and src.endswith("_c4_pmc.json")
    assert "nuts_gauss_dyn_kernel<8, false>" in json.load(open(os.path.join(ROOT, src)))["derived"]["kernel"]
    t2, why = bench.profiled_traffic(4, key, "nuts_gauss_no_such_kernel<8>")
    assert t2 is None and "not quoted" in why
    tm, srcm = bench.profiled_traffic(4, key, "nuts_gauss_memo_kernel<8, false, true>")    # what configs[3] runs on since round 6 (momenta from the pre-pass table)
    assert tm is not None and tm < t and "nuts_gauss_memo_kernel<8, false, true>" in json.load(open(os.path.join(ROOT, srcm)))["derived"]["kernel"]
    ti, whyi = bench.profiled_traffic(4, key, "nuts_gauss_memo_kernel<8, false, false>")   # the in-tick instantiation was never profiled under this name: no figure is made up
    assert ti is None and "not quoted" in whyi
    t3, why3 = bench.profiled_traffic(4, (4, 1234, 128, 200), "nuts_gauss_dyn_kernel<8, false>")
    assert t3 is None and "another workload shape" in why3


def test_gpus_flag_refuses_when_the_devices_are_not_there():
    """`bench.py --gpus 2` on a box with fewer than 2 visible GPUs: rc != 0 and no JSON line (it used to run one rank and print n_gpus 1)."""
    import torch
    if torch.cuda.is_available() and torch.cuda.device_count() >= 2:
        import pytest
        pytest.skip("two GPUs are visible here")
    env = {k: v for k, v in os.environ.items() if k not in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "BENCH_TEST_SHARE_GPU")}
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "2", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and not [l for l in out.stdout.splitlines() if l.startswith("{")]
    assert "refusing" in out.stderr


def test_gpus_flag_must_match_the_launcher():
    """Under a launcher (WORLD_SIZE set) a mismatching --gpus is an error, not a note on stderr."""
    env = dict(os.environ, WORLD_SIZE="1", RANK="0", LOCAL_RANK="0")
    out = subprocess.run([sys.executable, "bench.py", "--gpus", "4", "--steps", "1", "--warmup", "0"], cwd=ROOT, env=env,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode != 0 and not [l for l in out.stdout.splitlines() if l.startswith("{")]


def test_dump_outputs_writes_a_fixed_float64_sample(tmp_path):
    """--dump-outputs: the same seeded chains every time, draws capped (d = 512 x 100 kept draws: 81 chains), every chain's counts,
    everything float64 and under 64 MB."""
    import numpy as np
    import torch
    import bench
    C, d, n_keep, chain0 = 3000, 512, 100, 7
    draws = torch.arange(n_keep * d * C, dtype=torch.float64).view(n_keep, d, C)
    theta = -torch.arange(d * C, dtype=torch.float64).view(d, C)
    n_acc, n_leap, n_exec = (torch.arange(C, dtype=torch.int64) + k for k in (1, 2, 3))
    eps = torch.linspace(0.1, 0.2, C, dtype=torch.float64)
    for sub in ("a", "b"):
        bench.dump_outputs(str(tmp_path / sub), "nuts", C, chain0, d, n_keep, theta, draws, n_acc, n_leap, n_exec, eps)
    got = {p.stem: np.load(p) for p in (tmp_path / "a").iterdir()}
    assert sorted(got) == ["chain_ids", "draws", "n_accept", "n_leapfrogs", "n_leapfrogs_executed", "step_size", "theta"]
    assert all(a.dtype == np.float64 for a in got.values()) and sum(a.nbytes for a in got.values()) <= 64_000_000
    ids = got["chain_ids"].astype(np.int64) - chain0
    assert len(ids) == 81 and (np.diff(ids) > 0).all() and ids.max() < C
    assert np.array_equal(got["draws"], draws.numpy()[:, :, ids]) and np.array_equal(got["theta"], theta.numpy()[:, ids])
    assert np.array_equal(got["n_leapfrogs_executed"], n_exec.numpy()) and np.array_equal(got["step_size"], eps.numpy())
    for name, a in got.items():
        assert np.array_equal(a, np.load(tmp_path / "b" / (name + ".npy"))), name
