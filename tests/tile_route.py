"""Shared plumbing of the tile-route tests (include/mi_mcmc_tile_target.hpp): the two target libraries (examples/user_tile_target.hip and
tests/tile_targets.hip, each compiled once per process exactly as a user would), one call of a <name>_run entry point with every field of
mi_chains, and the oracle driven chain by chain by the library's host callback (test infrastructure: it drives the oracle)."""
import ctypes as C
import os
import subprocess
import tempfile

import numpy as np

import mcmc_amd
import orc
from mcmc_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
SOURCES = {"example": os.path.join(ROOT, "examples", "user_tile_target.hip"), "tests": os.path.join(ROOT, "tests", "tile_targets.hip")}
# NT -> (library, entry point, WPB of hmc_tile_kernel): the twisted Gaussian at every tile count
TWISTED = {1: ("tests", "twisted1_run", 4), 2: ("tests", "twisted2_run", 4), 4: ("example", "twisted_tile_run", 4), 8: ("tests", "twisted8_run", 8)}
ALGO = {"hmc": 0, "mala": 1, "nuts": 2}
ORC_ALGO = {"hmc": orc.ALGO_HMC, "mala": orc.ALGO_MALA, "nuts": orc.ALGO_NUTS}
B, S2 = 0.2, 1.5                                     # the twist of every test


class GaussTile(C.Structure):
    _fields_ = [("P", C.c_void_p), ("d", C.c_uint32)]


class TwistedTile(C.Structure):                      # TwistedTile of the example and TwistedTileN<NT, WPB> of tests/tile_targets.hip: one layout
    _fields_ = [("P", C.c_void_p), ("d", C.c_uint32), ("b", C.c_double), ("s2", C.c_double)]


_built = {}
_tmp = None


def hipcc_command(src, out, extra=()):
    return [HIPCC, "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "--offload-arch=gfx950", "-Wall", "-Werror", "-Wno-unused-function",
            *os.environ.get("MI_TILE_CFLAGS", "").split(), *extra, f"-I{ROOT}/include", "-shared", src,
            f"-L{ROOT}/mcmc_amd", "-lmi_mcmc", f"-Wl,-rpath,{ROOT}/mcmc_amd", "-o", out]


def build(which):
    """Path of the compiled library `which` ("example" / "tests"); one compile per process.  MI_TILE_PREBUILT names a directory that already holds
    lib<which>_tile_targets.so built by hipcc_command (a developer's shortcut when the same headers are tried many times)."""
    global _tmp
    if which in _built:
        return _built[which]
    pre = os.environ.get("MI_TILE_PREBUILT")
    if pre and os.path.exists(os.path.join(pre, f"lib{which}_tile_targets.so")):
        _built[which] = os.path.join(pre, f"lib{which}_tile_targets.so")
        return _built[which]
    if _tmp is None:
        _tmp = tempfile.TemporaryDirectory(prefix="tile_route_")
    out = os.path.join(_tmp.name, f"lib{which}_tile_targets.so")
    subprocess.check_call(hipcc_command(SOURCES[which], out))
    _built[which] = out
    return out


class Libs:
    """Both libraries, loaded after the engine (one HIP runtime for torch, the engine and the target libraries)."""

    def __init__(self):
        self.lib = {}
        self.host_kernel = self.get("tests").twisted_host_kernel_n

    def get(self, which):
        if which not in self.lib:
            path = build(which)
            mcmc_amd.lib()
            lib = self.lib[which] = C.CDLL(path)
            for name in ("twisted_host_kernel", "twisted_host_kernel_n"):
                if hasattr(lib, name): getattr(lib, name).restype = C.c_double
        return self.lib[which]

    def entry(self, nt):
        which, fn, _ = TWISTED[nt]
        return getattr(self.get(which), fn)


def have_toolchain():
    return os.path.exists(HIPCC) and os.path.exists(mcmc_amd.LIB_PATH)


def precision(d, seed=3):
    return synth.dense_gaussian_precision(d, seed=seed)


def mixed_bounds(d, seed, free=()):
    """A mix of the four bounds types of determine_bounds_type.hpp:27-57; the dimensions in `free` stay unbounded."""
    rng = np.random.default_rng(seed)
    kind = rng.integers(1, 5, d)
    kind[list(free)] = 1
    lb = np.where((kind == 2) | (kind == 4), -1.5, -np.inf)
    ub = np.where((kind == 3) | (kind == 4), 2.0, np.inf)
    return lb, ub


class Case:
    """One run of the twisted Gaussian on the tile route: everything both sides need."""

    def __init__(self, algo, nt, d, init, seed=4, burn=3, keep=6, L=4, eps=0.08, adapt=0, depth=6, lb=None, ub=None, M=None, chain0=0, pseed=3):
        assert 2 <= d <= 16 * nt
        self.algo, self.nt, self.d, self.init = algo, nt, d, np.ascontiguousarray(init, dtype=np.float64)
        self.seed, self.burn, self.keep, self.L, self.eps, self.adapt, self.depth = seed, burn, keep, L, eps, adapt, depth
        self.lb, self.ub, self.M, self.chain0 = lb, ub, M, chain0
        self.P = precision(d, pseed)
        self.C = self.init.shape[0]

    @property
    def gen(self):
        return self.lb is not None or self.M is not None

    def kernel_name(self):
        """mi_mcmc_last_kernel of this case (mala_tile_gen_kernel: mala_tile_kernel<T, true>)"""
        wpb = TWISTED[self.nt][2] if (self.algo == "hmc" and not self.gen) else 4
        return f"{self.algo}_tile{'_gen' if self.gen else ''}_kernel<user target, {wpb}>"

    def settings(self, burn=None, keep=None):
        kw = {}
        if self.lb is not None: kw.update(vals_bound=1, lower_bounds=self.lb, upper_bounds=self.ub)
        if self.M is not None: kw.update(precond_mat=self.M)
        return mcmc_amd.default_settings(rng_seed_value=self.seed, n_burnin_draws=self.burn if burn is None else burn,
                                         n_keep_draws=self.keep if keep is None else keep, n_leap_steps=self.L, step_size=self.eps,
                                         n_adapt_draws=self.adapt, max_tree_depth=self.depth, **kw)

    def orc_settings(self, burn=None, keep=None):
        kw = {}
        if self.lb is not None: kw.update(lower=self.lb, upper=self.ub)
        if self.M is not None: kw.update(precond=self.M)
        return orc.make_settings(seed=self.seed, n_burnin=self.burn if burn is None else burn, n_keep=self.keep if keep is None else keep,
                                 n_leap=self.L, step=self.eps, n_adapt=self.adapt, max_depth=self.depth, W=4, hoist=1, **kw)


def run_entry(fn, algo, target, d, init, st, chain0=0, draw0=0, eps_in=None, adapt_in=None, mem=mcmc_amd.MEM_HOST, stream=None,
              no_step_size=False, no_adapt_state=False):
    """One call of a MI_MCMC_DEFINE_TILE_TARGET entry point.  init [C, d].  no_step_size / no_adapt_state: a nuts call with these fields of mi_chains NULL.  Returns draws [n_keep, d, C] and the per-chain outputs (numpy, whatever
    `mem`).  A refusal raises mcmc_amd.MiMcmcError with the status code."""
    import torch
    Cn = init.shape[0]
    n_keep, n_tot = int(st.n_keep_draws), int(st.n_burnin_draws) + int(st.n_keep_draws)
    nuts = algo == 2
    host = dict(theta=np.ascontiguousarray(init.T.copy()), draws=np.zeros((n_keep, d, Cn)), n_accept=np.zeros(Cn, dtype=np.uint64),
                n_leap=np.zeros(Cn, dtype=np.uint64), eps=np.zeros(Cn) if eps_in is None else np.array(eps_in, dtype=np.float64, copy=True),
                depth=np.zeros((n_tot, Cn), dtype=np.uint32), adapt_state=np.zeros((3, Cn)) if adapt_in is None else np.array(adapt_in, dtype=np.float64, copy=True))
    if mem == mcmc_amd.MEM_DEVICE:
        as_t = lambda a: torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).cuda()
        buf = {k: as_t(v) for k, v in host.items()}
        torch.cuda.synchronize()                     # (uploaded on the default stream; the run goes to `stream`)
    else:
        buf = host
    ch = mcmc_amd.make_chains(buf["theta"], Cn, chain0=chain0, draws=buf["draws"], n_accept=buf["n_accept"], n_leapfrogs=buf["n_leap"],
                              step_size=buf["eps"] if nuts and not no_step_size else None, nuts_depth=buf["depth"] if nuts else None, mem=mem, draw0=draw0,
                              nuts_adapt_state=buf["adapt_state"] if nuts and not no_adapt_state else None)
    rc = fn(C.c_int(algo), C.byref(target), C.c_uint64(d), C.byref(st), C.byref(ch), C.c_void_p(stream or 0))
    if rc != 0:
        raise mcmc_amd.MiMcmcError(rc, mcmc_amd.lib().mi_mcmc_last_error().decode())
    torch.cuda.synchronize()
    if mem == mcmc_amd.MEM_DEVICE:
        for k, v in buf.items():
            host[k] = v.cpu().numpy().view(host[k].dtype)
    return host["draws"], host


def run_gpu(libs, case, burn=None, keep=None, init=None, draw0=0, eps_in=None, adapt_in=None, chain0=None, **kw):
    import torch
    Pd = torch.from_numpy(case.P).cuda()
    tgt = TwistedTile(Pd.data_ptr(), case.d, B, S2)
    out = run_entry(libs.entry(case.nt), ALGO[case.algo], tgt, case.d, case.init if init is None else init, case.settings(burn, keep),
                    chain0=case.chain0 if chain0 is None else chain0, draw0=draw0, eps_in=eps_in, adapt_in=adapt_in, **kw)
    del Pd
    return out


def run_gpu_cut(libs, case, cut):
    """The run of `case` in two calls, cut after `cut` of its burn + keep draws (cut > burn: both calls keep rows): the second call starts at the first's
    final theta with draw0 = cut, step_size and nuts_adapt_state handed over.  Returns what the uncut call returns."""
    assert case.burn < cut < case.burn + case.keep
    k1 = cut - case.burn
    a_draws, a = run_gpu(libs, case, keep=k1)
    b_draws, b = run_gpu(libs, case, burn=0, keep=case.keep - k1, init=a["theta"].T.copy(), draw0=cut,
                         eps_in=a["eps"] if case.algo == "nuts" else None, adapt_in=a["adapt_state"] if case.algo == "nuts" else None)
    out = dict(b)
    out["draws"] = np.concatenate([a_draws, b_draws])
    out["n_accept"] = a["n_accept"] + b["n_accept"]; out["n_leap"] = a["n_leap"] + b["n_leap"]
    out["depth"] = np.concatenate([a["depth"], b["depth"]])
    return out["draws"], out


def run_oracle(libs, case, chains=None, burn=None, keep=None, init=None):
    """The oracle, chain by chain (chain_id = chain0 + c), driven by the library's host callback.  chains: a subset (the other columns stay zero)."""
    s = case.orc_settings(burn, keep)
    n_keep, n_tot = int(s.n_keep_draws), int(s.n_burnin_draws) + int(s.n_keep_draws)
    init = case.init if init is None else init
    host = TwistedTile(case.P.ctypes.data, case.d, B, S2)
    Cn = init.shape[0]
    draws = np.zeros((n_keep, case.d, Cn))
    o = dict(n_accept=np.zeros(Cn, dtype=np.uint64), n_leap=np.zeros(Cn, dtype=np.uint64), eps=np.zeros(Cn), depth=np.zeros((n_tot, Cn), dtype=np.uint32))
    for c in (range(Cn) if chains is None else chains):
        s.chain_id = case.chain0 + c
        dr, info = orc.run_chain(ORC_ALGO[case.algo], None, init[c], s, traces=True, kernel=libs.host_kernel, data=C.addressof(host), d=case.d)
        draws[:, :, c] = dr; o["n_accept"][c] = info["n_accept"]; o["n_leap"][c] = info["n_leap"]; o["eps"][c] = info["eps"]; o["depth"][:, c] = info["depth"]
    if case.algo == "mala": o["n_leap"][:] = 0
    o["draws"] = draws
    return draws, o


def mismatches(algo, g_draws, g, o_draws, o, chains=None):
    """Names of the outputs that differ (bit-exact, NaN == NaN): draws, n_accept, and for nuts n_leap, eps and the depth trace."""
    sel = slice(None) if chains is None else list(chains)
    bad = []
    if not np.array_equal(g_draws[:, :, sel], o_draws[:, :, sel], equal_nan=True): bad.append("draws")
    if not np.array_equal(g["n_accept"][sel], o["n_accept"][sel]): bad.append("n_accept")
    if algo == "nuts":
        if not np.array_equal(g["n_leap"][sel], o["n_leap"][sel]): bad.append("n_leap")
        if not np.array_equal(g["eps"][sel], o["eps"][sel], equal_nan=True): bad.append("eps")
        if not np.array_equal(g["depth"][:, sel], o["depth"][:, sel]): bad.append("depth")
    return bad


def regime(o_draws, o):
    """Per chain of an oracle result: (finite throughout, accepted at least once)."""
    finite = np.isfinite(o_draws).all(axis=(0, 1)) & np.isfinite(o["eps"])
    return finite, o["n_accept"] > 0
