"""mcmc_amd -- host-side mirror of the C ABI in include/mi_mcmc.h (libmi_mcmc.so).

The product is the gfx950 shared library; this module only binds it (ctypes) so that tests,
bench.py and Python callers can reach `mi_mcmc_{hmc,mala,nuts}_run` with numpy / torch buffers.
Names follow the reference: settings fields are those of mcmc::algo_settings_t
(/root/reference/include/misc/mcmc_structs.hpp:66-101,123-134,151-184), the entry points those of
mcmc::hmc / mcmc::mala / mcmc::nuts (/root/reference/include/mcmc/{hmc,mala,nuts}.hpp).

There is no CPU fallback: if the library is missing, or no GPU is visible, calls raise.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import (EXPORTS, PROBE_EXPORTS,               # noqa: F401 -- the boundary as _abi states it, under the names this package has always had
                   MI_OK, MI_ERR_BAD_ARG, MI_ERR_HIP, MI_ERR_UNSUPPORTED, MI_ERR_OOM, MI_ERR_NO_DEVICE,
                   TARGET_GAUSS_ISO, TARGET_GAUSS_DIAG, TARGET_GAUSS_DENSE, TARGET_LOGISTIC, TARGET_NORMAL_MODEL, TARGET_GAUSS_MIXTURE,
                   MEM_HOST, MEM_DEVICE, KERNEL_AUTO, KERNEL_ELEMENTWISE_1LANE, KERNEL_ELEMENTWISE_4LANE, KERNEL_NUTS_LOCKSTEP,
                   KERNEL_HMC_TWO_WAVES_PER_SIMD, KERNEL_HMC_ONE_WAVE_PER_SIMD, KERNEL_HMC_SPLIT2, KERNEL_HMC_SPLIT4, KERNEL_HMC_SPLIT4_TWO_WAVES,
                   KERNEL_NUTS_TICK_LOCAL, KERNEL_NUTS_REG, KERNEL_NUTS_SPLIT, KERNEL_LITERAL, KERNEL_NUTS_DYN, KERNEL_NUTS_MEMO, KERNEL_NUTS_MEMO_INTICK,
                   STATS_ALL_LAGS, RANK_AVERAGE, RANK_NORMAL, RANK_SPLIT, RANK_FOLD, LOGLIK_ROWS, LOGLIK_SLAB, GEMM_PLAIN, GEMM_DENSE_M, GEMM_BOUNDED,
                   mi_target, mi_settings, mi_chains, mi_de_settings, mi_populations, mi_aees_settings, mi_aees_runs)


_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libmi_mcmc.so")


class MiMcmcError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__(f"mi_mcmc status {code}: {msg}")
        self.code = code


_lib = None


def _one_hip_runtime():
    """PyTorch-ROCm wheels bundle their own libamdhip64 / libhsa-runtime64 and dlopen them BY PATH on `import torch`.  If the
    engine was loaded first (bound to /opt/rocm's copies) the process would then hold two HIP runtimes, and torch's streams and
    device pointers mean nothing to the second one.  So: when torch is installed but not imported yet, load its runtime
    libraries first; the engine's DT_NEEDED entries (same sonames) then resolve to them, whichever import comes first."""
    import importlib.util
    import sys
    if "torch" in sys.modules:
        return
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.origin:
        return
    libdir = os.path.join(os.path.dirname(spec.origin), "lib")
    for name in ("libhsa-runtime64.so", "libamdhip64.so"):
        p = os.path.join(libdir, name)
        if os.path.exists(p):
            try:
                C.CDLL(p, mode=C.RTLD_GLOBAL)
            except OSError:
                pass


def lib():
    """Load libmi_mcmc.so (built in-tree by __graft_entry__.build() / mcmc_amd/csrc/Makefile)."""
    global _lib
    if _lib is None:
        path = os.environ.get("MI_MCMC_LIB", LIB_PATH)      # A/B builds of the same engine (tools/), never a fallback
        if not os.path.exists(path):
            raise MiMcmcError(-1, f"{path} not built: run `make -C mcmc_amd/csrc` (no CPU fallback)")
        _one_hip_runtime()
        _lib = _abi.declare(C.CDLL(path), _abi.EXPORTS + _abi.TEST_HOOKS, path)
    return _lib


_plib = None


def probes_lib():
    """Load libmi_mcmc_probes.so: the diagnostics of the GPU tests and tools/ (linked against the engine, loaded after it)."""
    global _plib
    if _plib is None:
        lib()
        path = os.path.join(os.path.dirname(LIB_PATH), "libmi_mcmc_probes.so")
        if not os.path.exists(path):
            raise MiMcmcError(-1, f"{path} not built: run `make -C mcmc_amd/csrc`")
        _plib = _abi.declare(C.CDLL(path), _abi.PROBE_EXPORTS, path)
    return _plib


def _check(rc):
    if rc != MI_OK:
        raise MiMcmcError(rc, lib().mi_mcmc_last_error().decode())


def _ptr(a):
    """Address of a numpy array (host), a torch tensor (host or device), an integer, or None: a Python int, what a pointer parameter takes."""
    if a is None or isinstance(a, int):
        return a
    if isinstance(a, np.integer):
        return int(a)
    if hasattr(a, "data_ptr"):
        return a.data_ptr()
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    raise TypeError(f"no address for a {type(a).__name__}: None, an integer, a numpy array or an object with data_ptr()")


def default_settings(**kw):
    """algo_settings_t with the reference defaults, then keyword overrides."""
    s = mi_settings()
    lib().mi_settings_default(C.byref(s))
    keep = []
    for k, v in kw.items():
        if k in ("lower_bounds", "upper_bounds", "precond_mat"):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.float64)
                keep.append(v)
                v = v.ctypes.data
        setattr(s, k, v)
    s._keep = keep
    return s


def make_target(kind, d, prec=None, X=None, y=None, mem=MEM_HOST, kernel_hint=KERNEL_AUTO):
    t = mi_target()
    t.struct_size = C.sizeof(mi_target)
    t.kind, t.d, t.mem, t.kernel_hint = kind, int(d), mem, int(kernel_hint)
    keep = []
    if mem == MEM_HOST:
        prec = None if prec is None else np.ascontiguousarray(prec, dtype=np.float64)
        X = None if X is None else np.ascontiguousarray(X, dtype=np.float64)
        y = None if y is None else np.ascontiguousarray(y, dtype=np.float64)
    keep += [prec, X, y]
    t.prec, t.X, t.y = _ptr(prec), _ptr(X), _ptr(y)
    t.n_rows = int(X.shape[0]) if X is not None else (int(y.shape[0]) if (y is not None and kind == TARGET_NORMAL_MODEL) else 0)
    t._keep = keep
    return t


def make_chains(theta, n_chains, chain0=0, draws=None, n_accept=None, step_size=None, n_leapfrogs=None,
                nuts_depth=None, mem=MEM_HOST, draw0=0, mass_diag=None, nuts_adapt_state=None, n_leapfrogs_executed=None):
    c = mi_chains()
    c.struct_size = C.sizeof(mi_chains)
    c.mem, c.n_chains, c.chain0, c.draw0 = mem, int(n_chains), int(chain0), int(draw0)
    c.theta, c.draws, c.n_accept = _ptr(theta), _ptr(draws), _ptr(n_accept)
    c.step_size, c.n_leapfrogs, c.nuts_depth = _ptr(step_size), _ptr(n_leapfrogs), _ptr(nuts_depth)
    c.mass_diag = _ptr(mass_diag)                         # hmc only: per-chain diagonal masses [d][C]
    c.nuts_adapt_state = _ptr(nuts_adapt_state)           # nuts: dual-averaging state [3][C], in (continuation inside the window) / out
    c.n_leapfrogs_executed = _ptr(n_leapfrogs_executed)   # out [C]: leapfrogs really computed (nuts on the memoised kernel: fewer than n_leapfrogs)
    c._keep = [theta, draws, n_accept, step_size, n_leapfrogs, nuts_depth, mass_diag, nuts_adapt_state, n_leapfrogs_executed]
    return c


_RUN = {"hmc": "mi_mcmc_hmc_run", "mala": "mi_mcmc_mala_run", "nuts": "mi_mcmc_nuts_run", "rwmh": "mi_mcmc_rwmh_run",
        "rmhmc": "mi_mcmc_rmhmc_run"}


def hmc_mass_adapted(target, settings, chains, n_windows=3, stream=None):
    """mi_mcmc_hmc_run_mass_adapted (NOT a reference mode): hmc with a diagonal mass matrix pooled over the chains and
    re-estimated after each of n_windows parts of the burn-in.  Returns the final mass diagonal [d]."""
    mass = np.zeros(int(target.d))
    _check(lib().mi_mcmc_hmc_run_mass_adapted(C.byref(target), C.byref(settings), C.byref(chains), n_windows, mass.ctypes.data, stream or 0))
    return mass


def _mass_adapted_dense(fn, target, settings, chains, n_windows, stream):
    d = int(target.d)
    M = np.zeros((d, d))
    _check(fn(C.byref(target), C.byref(settings), C.byref(chains), n_windows, M.ctypes.data, stream or 0))
    return M


def hmc_mass_adapted_dense(target, settings, chains, n_windows=3, stream=None):
    """mi_mcmc_hmc_run_mass_adapted_dense (NOT a reference mode): hmc with a DENSE mass matrix -- the shrunk, inverted pooled covariance of
    the chains' current states -- re-estimated after each of n_windows parts of the burn-in.  Returns the final matrix [d, d]."""
    return _mass_adapted_dense(lib().mi_mcmc_hmc_run_mass_adapted_dense, target, settings, chains, n_windows, stream)


def mala_mass_adapted_dense(target, settings, chains, n_windows=3, stream=None):
    """mi_mcmc_mala_run_mass_adapted_dense: the same for mala."""
    return _mass_adapted_dense(lib().mi_mcmc_mala_run_mass_adapted_dense, target, settings, chains, n_windows, stream)


def hmc_mass_adapted_per_chain(target, settings, chains, n_windows=3, mass_out=None, first_step_size=0.0, stream=None):
    """mi_mcmc_hmc_run_mass_adapted_per_chain (NOT a reference mode): every chain adapts its own diagonal mass from its own burn-in
    draws.  mass_out: [d][C] in the memory space of `chains` (numpy array or torch tensor) or None; first_step_size: the step of
    part 0 (M = I on the raw target; 0 = settings.step_size, which is in the preconditioned metric)."""
    _check(lib().mi_mcmc_hmc_run_mass_adapted_per_chain(C.byref(target), C.byref(settings), C.byref(chains), n_windows,
                                                        first_step_size, _ptr(mass_out), stream or 0))
    return mass_out


def rmhmc_callback(initial_vals, kernel_fn, kernel_data, tensor_fn, tensor_data, settings):
    """mi_mcmc_rmhmc_run_callback: mcmc::rmhmc for one chain with HOST callbacks.  kernel_fn / tensor_fn: C function pointers (ctypes
    function objects or raw addresses) with the signatures of mi_log_kernel_cb / mi_tensor_cb; *_data: addresses handed through.
    Returns (draws [n_keep, d], n_accept)."""
    x0 = np.ascontiguousarray(initial_vals, dtype=np.float64)
    d, n_keep = int(x0.shape[0]), int(settings.n_keep_draws)
    out = np.zeros((d, n_keep))                           # column-major n_keep x d
    nacc = C.c_uint64(0)
    _check(lib().mi_mcmc_rmhmc_run_callback(x0.ctypes.data, d, kernel_fn, kernel_data, tensor_fn, tensor_data, C.byref(settings),
                                            out.ctypes.data, C.byref(nacc)))
    return out.T.copy(), int(nacc.value)


def test_set_grid_cap(max_workgroups):
    """mi_mcmc_test_set_grid_cap (TEST HOOK, mi_mcmc_probes.h): cap the persistent grids of the dynamic-hand-out NUTS kernels and the grid-stride grids of the
    matrix-product route and of draws_predict (its pack and counting kernels); 0 = none."""
    lib().mi_mcmc_test_set_grid_cap(int(max_workgroups))


def test_set_linalg_stage_bytes(n_bytes):
    """mi_mcmc_test_set_linalg_stage_bytes (TEST HOOK, mi_mcmc_probes.h): the staging budget of the device INV (2 d doubles) / CHOL_LOWER (d doubles)
    in bytes, beyond which a matrix runs the host loops; 0 = the real budget (60 KB of LDS).  Empties the memoised factorisations."""
    lib().mi_mcmc_test_set_linalg_stage_bytes(int(n_bytes))


def test_linalg_computed():
    """mi_mcmc_test_linalg_computed (TEST HOOK, mi_mcmc_probes.h): INV / CHOL_LOWER factorisations computed so far, i.e. not answered by the memo."""
    return lib().mi_mcmc_test_linalg_computed()


def test_linalg_computed_on_device():
    """mi_mcmc_test_linalg_computed_on_device (TEST HOOK, mi_mcmc_probes.h): ... those of them that ran the device kernels, not the host loops."""
    return lib().mi_mcmc_test_linalg_computed_on_device()


def test_set_gemm_nuts_ws_bytes(n_bytes):
    """mi_mcmc_test_set_gemm_nuts_ws_bytes (TEST HOOK, mi_mcmc_probes.h): the workspace nuts on the matrix-product route may take for itself (the packed matrices
    and one range of chains), as if that were all the free device memory; 0 = the real figure.  Fewer chains than the call's fit: consecutive ranges in multiples of
    128; not even 128: the literal kernel.  Results do not depend on it."""
    lib().mi_mcmc_test_set_gemm_nuts_ws_bytes(int(n_bytes))


def test_gemm_nuts_ranges():
    """mi_mcmc_test_gemm_nuts_ranges (TEST HOOK): ranges of chains nuts on the matrix-product route has run so far in this process (monotonic)."""
    return lib().mi_mcmc_test_gemm_nuts_ranges()


def test_gemm_nuts_last_ticks():
    """mi_mcmc_test_gemm_nuts_last_ticks (TEST HOOK): of the last nuts call on the matrix-product route -- ticks run, (tick, chain) slots in which the chain was
    not idle, and all (tick, chain) slots."""
    t, b, n = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    lib().mi_mcmc_test_gemm_nuts_last_ticks(C.byref(t), C.byref(b), C.byref(n))
    return int(t.value), int(b.value), int(n.value)


def test_gemm_nuts_tick_ceiling(max_tree_depth, n_draws, search=True):
    """mi_mcmc_test_gemm_nuts_tick_ceiling (TEST HOOK; host arithmetic, no device): the ticks after which the route's host loop gives up."""
    return lib().mi_mcmc_test_gemm_nuts_tick_ceiling(int(max_tree_depth), int(n_draws), 1 if search else 0)


def test_gemm_nuts_chain_bytes(d, n_rows, max_tree_depth):
    """mi_mcmc_test_gemm_nuts_chain_bytes (TEST HOOK; host arithmetic): workspace bytes per chain; n_rows = 0: the dense Gaussian."""
    return lib().mi_mcmc_test_gemm_nuts_chain_bytes(int(d), int(n_rows), int(max_tree_depth))


def test_gemm_nuts_bounded_chain_bytes(d, n_rows, max_tree_depth):
    """mi_mcmc_test_gemm_nuts_bounded_chain_bytes (TEST HOOK; host arithmetic): workspace bytes per chain of a call with vals_bound -- one vector of padded d doubles
    more than test_gemm_nuts_chain_bytes (theta of the last point next to x)."""
    return lib().mi_mcmc_test_gemm_nuts_bounded_chain_bytes(int(d), int(n_rows), int(max_tree_depth))


def test_gemm_nuts_fixed_bytes(d, n_rows):
    """mi_mcmc_test_gemm_nuts_fixed_bytes (TEST HOOK; host arithmetic): workspace bytes that do not depend on the chains (the packed matrices, the counters)."""
    return lib().mi_mcmc_test_gemm_nuts_fixed_bytes(int(d), int(n_rows))


def test_gemm_nuts_range_chains(n_chains, chain_bytes, fixed_bytes, budget):
    """mi_mcmc_test_gemm_nuts_range_chains (TEST HOOK; host arithmetic): chains per range under `budget` bytes -- all of them (padded to 128) or a multiple of 128; 0: none."""
    return lib().mi_mcmc_test_gemm_nuts_range_chains(int(n_chains), int(chain_bytes), int(fixed_bytes), int(budget))


def test_set_gemm_graph(mode):
    """mi_mcmc_test_set_gemm_graph (TEST HOOK, mi_mcmc_probes.h): 1 = the samplers of the matrix-product route never capture the launches of a draw / a tick into a
    graph (what a call of 65 536 chains does); 0 = the rule as it is.  Results do not depend on it."""
    lib().mi_mcmc_test_set_gemm_graph(int(mode))


def test_set_gemm_ws_bytes(n_bytes):
    """mi_mcmc_test_set_gemm_ws_bytes (TEST HOOK, mi_mcmc_probes.h): the device memory the capacity condition of hmc / mala / rwmh on the matrix-product route sees
    (0 = the real figure); a call that needs more stays on the literal kernel.  Results do not depend on it."""
    lib().mi_mcmc_test_set_gemm_ws_bytes(int(n_bytes))


def test_gemm_need_bytes(d, n_rows, n_chains, variant=GEMM_PLAIN, replay=True):
    """mi_mcmc_test_gemm_need_bytes (TEST HOOK; host arithmetic, no device): what that condition compares with the memory -- the workspace, with `replay` (hmc, mala)
    the literal replay's part behind it, and the uploads.  n_rows = 0: the dense Gaussian."""
    return lib().mi_mcmc_test_gemm_need_bytes(int(d), int(n_rows), int(n_chains), int(variant), 1 if replay else 0)


def last_kernel():
    """mi_mcmc_last_kernel: the kernel this thread's last run spent its time in, as rocprofv3 names it."""
    return lib().mi_mcmc_last_kernel().decode()


def release_workspace(stream=None, all_streams=True):
    """mi_mcmc_release_workspace: free the cached kernel workspaces of the current device; returns the bytes freed."""
    n = C.c_uint64(0)
    _check(lib().mi_mcmc_release_workspace(stream or 0, 1 if all_streams else 0, C.byref(n)))
    return int(n.value)


def run(algo, target, settings, chains, stream=None):
    """Raw call: mi_mcmc_<algo>_run(target, settings, chains, stream)."""
    fn = getattr(lib(), _RUN[algo])
    _check(fn(C.byref(target), C.byref(settings), C.byref(chains), stream or 0))


def sample(algo, kind, init, settings, prec=None, X=None, y=None, chain0=0, want_draws=True, draw0=0, step_size_in=None,
           kernel_hint=KERNEL_AUTO, adapt_state_in=None, want_adapt_state=False):
    """Host-buffer convenience: init is [C, d] (row per chain, like C calls of mcmc::<algo> with
    initial_vals = init[c]).  Returns draws [n_keep, d, C] and a dict of per-chain outputs."""
    init = np.ascontiguousarray(init, dtype=np.float64)
    n_chains, d = init.shape
    theta = np.array(init.T, dtype=np.float64, order="C", copy=True)   # [d][C]; always a copy (the run overwrites it)
    n_keep = int(settings.n_keep_draws)
    draws = np.zeros((n_keep, d, n_chains)) if want_draws else None
    n_accept = np.zeros(n_chains, dtype=np.uint64)
    n_leap = np.zeros(n_chains, dtype=np.uint64)
    eps = np.zeros(n_chains) if step_size_in is None else np.array(step_size_in, dtype=np.float64, copy=True)
    n_tot = int(settings.n_burnin_draws) + n_keep
    depth = np.zeros((n_tot, n_chains), dtype=np.uint32) if algo == "nuts" else None
    adapt = None
    if algo == "nuts" and (want_adapt_state or adapt_state_in is not None):    # the dual-averaging state [3][C]: in (continuation inside the window) / out
        adapt = np.zeros((3, n_chains)) if adapt_state_in is None else np.array(adapt_state_in, dtype=np.float64, copy=True)
    t = make_target(kind, d, prec=prec, X=X, y=y, kernel_hint=kernel_hint)
    n_exec = np.zeros(n_chains, dtype=np.uint64)
    c = make_chains(theta, n_chains, chain0=chain0, draws=draws, n_accept=n_accept,
                    step_size=eps, n_leapfrogs=n_leap, nuts_depth=depth, draw0=draw0, nuts_adapt_state=adapt, n_leapfrogs_executed=n_exec)
    run(algo, t, settings, c)
    return draws, dict(n_accept=n_accept, n_leap=n_leap, eps=eps, theta=theta, depth=depth, adapt_state=adapt, n_exec=n_exec)


def sample_device(algo, kind, init, settings, prec=None, X=None, y=None, chain0=0, want_draws=True, draw0=0,
                  step_size_in=None, kernel_hint=KERNEL_AUTO, device=None, stream=None):
    """Device-resident form of sample(): chain state, draws and counters are torch tensors in HBM on `device` (default:
    the current CUDA device) and stay there -- what mcmc_amd.dist all-gathers over RCCL without a host round trip.
    init: [C, d] numpy array or torch tensor.  Returns (draws [n_keep, d, C] or None, dict of per-chain tensors)."""
    import torch
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    with torch.cuda.device(dev):
        init_t = torch.as_tensor(init, dtype=torch.float64).to(dev)
        n_chains, d = init_t.shape
        theta = init_t.t().contiguous()                                    # [d][C]; a copy (the run overwrites it)
        if theta.data_ptr() == init_t.data_ptr():
            theta = theta.clone()
        n_keep = int(settings.n_keep_draws)
        n_tot = int(settings.n_burnin_draws) + n_keep
        draws = torch.empty((n_keep, d, n_chains), dtype=torch.float64, device=dev) if want_draws else None
        n_accept = torch.zeros(n_chains, dtype=torch.int64, device=dev)
        n_leap = torch.zeros(n_chains, dtype=torch.int64, device=dev)
        eps = (torch.zeros(n_chains, dtype=torch.float64, device=dev) if step_size_in is None
               else torch.as_tensor(step_size_in, dtype=torch.float64).to(dev).clone())
        depth = torch.zeros((n_tot, n_chains), dtype=torch.int32, device=dev) if algo == "nuts" else None
        to_dev = lambda a: None if a is None else torch.as_tensor(a, dtype=torch.float64).to(dev).contiguous()
        t = make_target(kind, d, prec=to_dev(prec), X=to_dev(X), y=to_dev(y), mem=MEM_DEVICE, kernel_hint=kernel_hint)
        c = make_chains(theta, n_chains, chain0=chain0, draws=draws, n_accept=n_accept, step_size=eps,
                        n_leapfrogs=n_leap, nuts_depth=depth, mem=MEM_DEVICE, draw0=draw0)
        st = torch.cuda.current_stream(dev).cuda_stream if stream is None else stream
        run(algo, t, settings, c, stream=st)
    return draws, dict(n_accept=n_accept, n_leap=n_leap, eps=eps, theta=theta, depth=depth)


# mcmc::hmc / mcmc::mala / mcmc::nuts, many chains at once
def hmc(kind, init, settings, **kw):
    return sample("hmc", kind, init, settings, **kw)


def mala(kind, init, settings, **kw):
    return sample("mala", kind, init, settings, **kw)


def nuts(kind, init, settings, **kw):
    return sample("nuts", kind, init, settings, **kw)


def rwmh(kind, init, settings, **kw):
    """mcmc::rwmh: settings.step_size carries par_scale, settings.precond_mat carries cov_mat."""
    return sample("rwmh", kind, init, settings, **kw)


def rmhmc(kind, init, settings, **kw):
    """mcmc::rmhmc with the metric tensor built into the target kind (TARGET_NORMAL_MODEL: Fisher information)."""
    return sample("rmhmc", kind, init, settings, **kw)


LOG_KERNEL_CB = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double), C.c_void_p)


def hmc_callback(initial_vals, callback, settings, target_data=None, algo="hmc"):
    """mcmc::hmc / mala / nuts with a host callback for one chain (mi_mcmc_<algo>_run_callback).

    callback: either a ctypes function pointer with the mi_log_kernel_cb signature or a Python
    callable f(vals: np.ndarray, want_grad: bool) -> (value, grad or None)."""
    x0 = np.ascontiguousarray(initial_vals, dtype=np.float64)
    d = x0.size
    n_keep = int(settings.n_keep_draws)
    draws = np.zeros((n_keep, d), order="F")
    n_acc = C.c_uint64(0)
    if callable(callback) and not isinstance(callback, C._CFuncPtr):
        def _tramp(vals, grad, _user):
            v = np.ctypeslib.as_array(vals, shape=(d,))
            val, g = callback(v.copy(), bool(grad))
            if grad:
                np.ctypeslib.as_array(grad, shape=(d,))[:] = g
            return float(val)
        cb = LOG_KERNEL_CB(_tramp)
    else:
        cb = callback
    fn = getattr(lib(), f"mi_mcmc_{algo}_run_callback")
    args = [x0.ctypes.data, d, cb, target_data or 0, C.byref(settings), draws.ctypes.data, C.byref(n_acc)]
    if algo == "nuts":
        args.append(None)
    _check(fn(*args))
    return draws, int(n_acc.value)


def mala_callback(initial_vals, callback, settings, target_data=None):
    return hmc_callback(initial_vals, callback, settings, target_data, algo="mala")


def nuts_callback(initial_vals, callback, settings, target_data=None):
    return hmc_callback(initial_vals, callback, settings, target_data, algo="nuts")


def rwmh_callback(initial_vals, callback, settings, target_data=None):
    """settings.step_size carries par_scale; the callback is asked for the value only"""
    return hmc_callback(initial_vals, callback, settings, target_data, algo="rwmh")


def de_settings(**kw):
    """de_settings_t with the reference defaults (jumps false, n_pop 100, par_b 1e-4, par_gamma_jump 2), then keyword overrides;
    initial_lb / initial_ub: d values (the initial box of every population) or None."""
    s = mi_de_settings()
    lib().mi_de_settings_default(C.byref(s))
    keep = []
    for k, v in kw.items():
        if k in ("initial_lb", "initial_ub"):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.float64)
                keep.append(v)
                v = v.ctypes.data
        setattr(s, k, v)
    s._keep = keep
    return s


def de(kind, init, settings, de_settings=None, n_pop=None, prec=None, X=None, y=None, population0=0, draw0=0, population=None,
       want_draws=True, kernel_hint=KERNEL_AUTO):
    """mcmc::de for P populations at once (mi_mcmc_de_run), host buffers.  init: [P, d] (initial_vals of every population);
    settings: rng_seed_value, bounds, n_burnin_draws / n_keep_draws; de_settings: mi_de_settings (n_pop overrides its n_pop).
    population: [n_pop, d, P] to continue a run (draw0 > 0).  Returns draws [n_keep, n_pop, d, P] (or None) and a dict with the
    final population [n_pop, d, P] (transformed space) and n_accept [P]."""
    ds = de_settings if de_settings is not None else globals()["de_settings"]()
    if n_pop is not None:
        ds.n_pop = int(n_pop)
    init = np.ascontiguousarray(init, dtype=np.float64)
    P, d = init.shape
    iv = np.ascontiguousarray(init.T)                                    # [d][P]
    npop, n_keep = int(ds.n_pop), int(settings.n_keep_draws)
    pop = np.zeros((npop, d, P)) if population is None else np.array(population, dtype=np.float64, order="C", copy=True)
    draws = np.zeros((n_keep, npop, d, P)) if want_draws else None
    n_accept = np.zeros(P, dtype=np.uint64)
    t = make_target(kind, d, prec=prec, X=X, y=y, kernel_hint=kernel_hint)
    p = mi_populations()
    p.struct_size = C.sizeof(mi_populations)
    p.mem, p.n_populations, p.population0, p.draw0 = MEM_HOST, P, int(population0), int(draw0)
    p.initial_vals, p.population, p.draws, p.n_accept = _ptr(iv), _ptr(pop), _ptr(draws), _ptr(n_accept)
    _check(lib().mi_mcmc_de_run(C.byref(t), C.byref(settings), C.byref(ds), C.byref(p), None))
    return draws, dict(population=pop, n_accept=n_accept)


def de_callback(initial_vals, callback, settings, de_settings=None, n_pop=None, target_data=None):
    """mcmc::de with a host callback for one population (mi_mcmc_de_run_callback).  callback: a ctypes mi_log_kernel_cb or a
    Python callable f(vals: np.ndarray) -> value.  Returns draws [n_keep, n_pop, d] and n_accept."""
    ds = de_settings if de_settings is not None else globals()["de_settings"]()
    if n_pop is not None:
        ds.n_pop = int(n_pop)
    x0 = np.ascontiguousarray(initial_vals, dtype=np.float64)
    d = x0.size
    draws = np.zeros((int(settings.n_keep_draws), int(ds.n_pop), d))
    n_acc = C.c_uint64(0)
    if callable(callback) and not isinstance(callback, C._CFuncPtr):
        def _tramp(vals, _grad, _user):
            return float(callback(np.ctypeslib.as_array(vals, shape=(d,)).copy()))
        cb = LOG_KERNEL_CB(_tramp)
    else:
        cb = callback
    _check(lib().mi_mcmc_de_run_callback(x0.ctypes.data, d, cb, target_data or 0, C.byref(settings), C.byref(ds), draws.ctypes.data, C.byref(n_acc)))
    return draws, int(n_acc.value)


def mixture_log_constants(weights, variances, d):
    """log c_i = log w_i - (d / 2) log(2 pi s2_i): the y of a TARGET_GAUSS_MIXTURE (include/mi_mcmc.h)"""
    w = np.asarray(weights, dtype=np.float64)
    s2 = np.asarray(variances, dtype=np.float64)
    return np.log(w) - (d / 2.0) * np.log(2.0 * np.pi * s2)


def mixture_target(means, variances, weights, mem=MEM_HOST):
    """TARGET_GAUSS_MIXTURE: means [M, d], variances [M] (isotropic per component), weights [M]"""
    means = np.ascontiguousarray(means, dtype=np.float64)
    M, d = means.shape
    return make_target(TARGET_GAUSS_MIXTURE, d, prec=np.asarray(variances, dtype=np.float64).reshape(M), X=means,
                       y=mixture_log_constants(weights, variances, d), mem=mem)


def aees_settings(**kw):
    """aees_settings_t with the reference defaults (n_initial_draws 1000, par_scale 1, n_rings 5, ee_prob_par 0.1, no temper_vec),
    then keyword overrides; cov_mat: d x d or None (identity); temper_vec: the temperatures above 1 (any order) or None."""
    s = mi_aees_settings()
    lib().mi_aees_settings_default(C.byref(s))
    keep = []
    for k, v in kw.items():
        if k in ("cov_mat", "temper_vec"):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=np.float64).reshape(-1)
                keep.append(v)
                if k == "temper_vec":
                    s.temper_len = v.size
                v = v.ctypes.data
            elif k == "temper_vec":
                s.temper_len = 0
        setattr(s, k, v)
    s._keep = keep
    return s


def aees(target, init, settings, aees_settings=None, run0=0, want_draws=True):
    """mcmc::aees for P independent runs at once (mi_mcmc_aees_run), host buffers.  target: a mi_target (make_target /
    mixture_target) or a kind (then a Gaussian with no parameters, TARGET_GAUSS_ISO); init: [P, d]; settings: rng_seed_value,
    bounds, n_burnin_draws / n_keep_draws.  Returns draws [n_keep, d, P] (or None) and a dict with final_states [K, d, P]
    (transformed space), n_accept [K, P] and n_ee_accept [K, P]."""
    a = aees_settings if aees_settings is not None else globals()["aees_settings"]()
    init = np.ascontiguousarray(init, dtype=np.float64)
    P, d = init.shape
    t = make_target(target, d) if isinstance(target, int) else target
    K, n_keep = int(a.temper_len) + 1, int(settings.n_keep_draws)
    iv = np.ascontiguousarray(init.T)                                    # [d][P]
    draws = np.zeros((n_keep, d, P)) if want_draws else None
    fin = np.zeros((K, d, P))
    n_acc = np.zeros((K, P), dtype=np.uint64)
    n_ee = np.zeros((K, P), dtype=np.uint64)
    r = mi_aees_runs()
    r.struct_size = C.sizeof(mi_aees_runs)
    r.mem, r.n_runs, r.run0 = MEM_HOST, P, int(run0)
    r.initial_vals, r.draws, r.final_states, r.n_accept, r.n_ee_accept = _ptr(iv), _ptr(draws), _ptr(fin), _ptr(n_acc), _ptr(n_ee)
    _check(lib().mi_mcmc_aees_run(C.byref(t), C.byref(settings), C.byref(a), C.byref(r), None))
    return draws, dict(final_states=fin, n_accept=n_acc, n_ee_accept=n_ee)


def aees_callback(initial_vals, callback, settings, aees_settings=None, target_data=None):
    """mcmc::aees with a host callback for one run (mi_mcmc_aees_run_callback).  callback: a ctypes mi_log_kernel_cb or a Python
    callable f(vals: np.ndarray) -> value.  Returns draws [n_keep, d] and a dict with final_states [K, d], n_accept [K], n_ee_accept [K]."""
    a = aees_settings if aees_settings is not None else globals()["aees_settings"]()
    x0 = np.ascontiguousarray(initial_vals, dtype=np.float64)
    d, K = x0.size, int(a.temper_len) + 1
    draws = np.zeros((int(settings.n_keep_draws), d))
    fin = np.zeros((K, d))
    n_acc = np.zeros(K, dtype=np.uint64)
    n_ee = np.zeros(K, dtype=np.uint64)
    if callable(callback) and not isinstance(callback, C._CFuncPtr):
        def _tramp(vals, _grad, _user):
            return float(callback(np.ctypeslib.as_array(vals, shape=(d,)).copy()))
        cb = LOG_KERNEL_CB(_tramp)
    else:
        cb = callback
    _check(lib().mi_mcmc_aees_run_callback(x0.ctypes.data, d, cb, target_data or 0, C.byref(settings), C.byref(a), draws.ctypes.data, fin.ctypes.data,
                                           n_acc.ctypes.data, n_ee.ctypes.data))
    return draws, dict(final_states=fin, n_accept=n_acc, n_ee_accept=n_ee)


# ---------------------------------------------------------------- diagnostics (GPU tests)
def probe_mfma(A, B, Cin):
    A = np.ascontiguousarray(A, dtype=np.float64)
    B = np.ascontiguousarray(B, dtype=np.float64)
    Cin = np.ascontiguousarray(Cin, dtype=np.float64)
    D = np.zeros((16, 16))
    _check(probes_lib().mi_probe_mfma_f64(A.ctypes.data, B.ctypes.data, Cin.ctypes.data, D.ctypes.data))
    return D


def probe_math(fn, x, kc2=False):
    """fn 0..5: exp, log, sincos2pi (sin, cos), softplus, sigmoid, norm_ppf on the device; kc2: from the unit built with MI_KC_MODE 2 (probes_kc2.hip)"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    o1, o2 = np.empty_like(x), np.empty_like(x)
    f = probes_lib().mi_probe_math_kc2 if kc2 else probes_lib().mi_probe_math
    _check(f(fn, x.ctypes.data, x.size, o1.ctypes.data, o2.ctypes.data))
    return o1, o2


def probe_math2(fn, x, y, kc2=False):
    """fn 0: det_pow(x, y) on the device, elementwise over two arrays of one shape"""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.ascontiguousarray(y, dtype=np.float64)
    if x.shape != y.shape:
        raise ValueError(f"probe_math2: x {x.shape} and y {y.shape} differ in shape")
    out = np.empty_like(x)
    f = probes_lib().mi_probe_math2_kc2 if kc2 else probes_lib().mi_probe_math2
    _check(f(fn, x.ctypes.data, y.ctypes.data, x.size, out.ctypes.data))
    return out


def probe_normals(seed, chain, draw, stream, d):
    out = np.zeros(d)
    _check(probes_lib().mi_probe_normals(seed, chain, draw, stream, d, out.ctypes.data))
    return out


def probe_normals_variant(variant, seed, chain, draw, stream, d, kc2=False):
    """the same d normals through variant 0 rng_normal_pair, 1 rng_normal_pair_at, 2 rng_normal_two_pairs, 3 rng_normal_four_pairs"""
    out = np.zeros(d)
    if kc2:
        _check(probes_lib().mi_probe_normals_kc2(variant, seed, chain, draw, stream, d, out.ctypes.data))
    else:
        _check(probes_lib().mi_probe_normals_variant(variant, seed, chain, draw, stream, d, out.ctypes.data))
    return out


def probe_uniform(seed, chain, draw, slot):
    out = np.zeros(1)
    _check(probes_lib().mi_probe_uniform(seed, chain, draw, slot, out.ctypes.data))
    return float(out[0])


def probe_fp64_peak(use_mfma, iters=20000):
    out = C.c_double(0.0)
    _check(probes_lib().mi_probe_fp64_peak(int(use_mfma), int(iters), C.byref(out)))
    return out.value


def probe_mfma_cycles(waves_per_simd, use_lds, iters=20000):
    cyc, tf = C.c_double(0.0), C.c_double(0.0)
    _check(probes_lib().mi_probe_mfma_cycles(int(waves_per_simd), int(use_lds), int(iters), C.byref(cyc), C.byref(tf)))
    return cyc.value, tf.value


def mat_inverse(A):
    """INV of a d x d matrix as the engine computes it for a dense precond_mat (mi_mcmc_mat_inverse: the oracle's operation order; d >= 64 on the device)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    d = A.shape[0]
    out = np.empty((d, d))
    _check(lib().mi_mcmc_mat_inverse(A.ctypes.data, d, out.ctypes.data))
    return out


def mat_cholesky_lower(A):
    """CHOL_LOWER likewise (mi_mcmc_mat_cholesky_lower)."""
    A = np.ascontiguousarray(A, dtype=np.float64)
    d = A.shape[0]
    out = np.empty((d, d))
    _check(lib().mi_mcmc_mat_cholesky_lower(A.ctypes.data, d, out.ctypes.data))
    return out


def draw_stats(draws, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, want_acov=True):
    """mi_mcmc_draw_stats: pooled mean [d], autocovariance [n_keep, d], R-hat [d] and per-chain ESS [d] of a draws slab
    [n_keep, d, C] (numpy array, or a device tensor / pointer with mem=MEM_DEVICE and explicit shape).  want_acov=False: ESS and
    R-hat only -- as many lags as Geyer's sum needs, straight from HBM (acov is None in the result)."""
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        n_keep, d, n_chains = draws.shape
    mean = np.zeros(d)
    acov = np.zeros((n_keep, d)) if want_acov else None
    rhat, ess = np.zeros(d), np.zeros(d)
    _check(lib().mi_mcmc_draw_stats(_ptr(draws), mem, n_keep, d, n_chains, mean.ctypes.data, _ptr(acov), rhat.ctypes.data, ess.ctypes.data, stream or 0))
    return dict(mean=mean, acov=acov, rhat=rhat, ess=ess)


def test_draw_stats_last():
    """mi_mcmc_test_draw_stats_last (TEST HOOK, mi_mcmc_probes.h): what this thread's last draw_stats call launched -- a dict of route (0 the one-pass Gram
    kernel, 1 the window + lag-block ladder, 2 the streamed kernel), NB, G, tiles (64-chain tiles of the largest chain group), window_launches, lag_passes,
    subset_passes, smallest_subset."""
    o = (C.c_uint64 * 8)()
    lib().mi_mcmc_test_draw_stats_last(o)
    return dict(zip(("route", "NB", "G", "tiles", "window_launches", "lag_passes", "subset_passes", "smallest_subset"), (int(v) for v in o)))


def test_stats_host(acov=None, n=None, moments=None, n_chains=None):
    """mi_mcmc_test_stats_host (TEST HOOK, mi_mcmc_probes.h): the host arithmetic draw_stats and draw_stats_lags share, no device.  acov [nlag, d] of series
    of n draws -> ess [d], hit [d] (uint8: Geyer's sum over the lags [0, nlag) met its non-positive pair); moments [G, d, 3] of n_chains chains of n draws
    -> rhat [d].  Returns a dict; what was not asked for is None."""
    ess = hit = rhat = None
    nlag = d = G = 0
    if acov is not None:
        acov = np.ascontiguousarray(acov, dtype=np.float64)
        nlag, d = acov.shape
        ess, hit = np.zeros(d), np.zeros(d, dtype=np.uint8)
    if moments is not None:
        moments = np.ascontiguousarray(moments, dtype=np.float64)
        G, d = moments.shape[:2]
        rhat = np.zeros(d)
    lib().mi_mcmc_test_stats_host(_ptr(acov), nlag, d, int(n), _ptr(moments), G, int(n_chains or 0), _ptr(ess), _ptr(hit), _ptr(rhat))
    return dict(ess=ess, hit=hit, rhat=rhat)


def draw_stats_lags(draws, max_lag=None, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, want_acov=True):
    """mi_mcmc_draw_stats_lags: pooled mean [d], autocovariance [K + 1, d] with K = min(max_lag, n_keep - 1) (max_lag=None: every lag), R-hat [d],
    per-chain ESS [d] over the lags [0, K] and ended [d] (uint8; 0: the window cut Geyer's sum) of a draws slab [n_keep, d, C] of any length, on the
    fp64 matrix cores (numpy array, or a device tensor / pointer with mem=MEM_DEVICE and explicit shape).  want_acov=False: further bands of lags run
    only over the dimensions whose sum is still open (acov is None in the result); the other outputs have the same bits.  mcmc_amd.acov is the
    numpy statement."""
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        n_keep, d, n_chains = draws.shape
    n_keep, d, n_chains = int(n_keep), int(d), int(n_chains)
    ml = STATS_ALL_LAGS if max_lag is None else int(max_lag)
    K = min(ml, max(n_keep, 1) - 1)
    mean, rhat, ess, ended = np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d, dtype=np.uint8)
    acov = np.zeros((K + 1, d)) if want_acov else None
    _check(lib().mi_mcmc_draw_stats_lags(_ptr(draws), mem, n_keep, d, n_chains, ml, mean.ctypes.data, _ptr(acov), rhat.ctypes.data,
                                         ess.ctypes.data, ended.ctypes.data, stream or 0))
    return dict(mean=mean, acov=acov, rhat=rhat, ess=ess, ended=ended)


def test_draw_stats_lags_last():
    """mi_mcmc_test_draw_stats_lags_last (TEST HOOK, mi_mcmc_probes.h): what this thread's last draw_stats_lags call launched -- a dict of ND (block
    offsets), bands, subset_passes (band passes over a subset of the dimensions), smallest_subset, time_tiles (per series), G (chain groups),
    tile_chains, K."""
    o = (C.c_uint64 * 8)()
    lib().mi_mcmc_test_draw_stats_lags_last(o)
    return dict(zip(("ND", "bands", "subset_passes", "smallest_subset", "time_tiles", "G", "tile_chains", "K"), (int(v) for v in o)))


def draws_covariance(draws, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, want_mean=True, want_cov=True):
    """mi_mcmc_draws_covariance: pooled mean [d] and covariance [d, d] of the n_keep * C columns of a slab [n_keep, d, C] (numpy array -- a
    2-D [d, C] array is the case n_keep = 1, the chains' state --, or a device tensor / pointer with mem=MEM_DEVICE and explicit shape).
    Returns (mean, cov); an output that is not wanted is None."""
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 2:
            draws = draws[None]
        n_keep, d, n_chains = draws.shape
    mean = np.zeros(d) if want_mean else None
    cov = np.zeros((d, d)) if want_cov else None
    _check(lib().mi_mcmc_draws_covariance(_ptr(draws), mem, n_keep, d, n_chains, _ptr(mean), _ptr(cov), stream or 0))
    return mean, cov


def _slab_shape(draws, n_keep, d, n_chains, mem):
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 2:
            draws = draws[None]
        n_keep, d, n_chains = draws.shape
    return draws, int(n_keep), int(d), int(n_chains)


def draw_stats_nested(draws, chains_per_super, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, want_nrhat=True, want_mean=True,
                      want_between=True, want_within=True, want_mcse_mean=True, want_super_mean=True):
    """mi_mcmc_draw_stats_nested: the nested R-hat of a slab [n_keep, d, C] whose C chains are K = C // chains_per_super superchains of chains_per_super
    consecutive chains started from one point (Margossian et al. 2024; numpy array -- a 2-D [d, C] array is the case n_keep = 1, the chains' state --,
    or a device tensor / pointer with mem=MEM_DEVICE and explicit shape).  Returns a dict of nrhat, mean, between, within, mcse_mean [d] and
    super_mean [K, d]; an output that is not wanted is None.  mcmc_amd.nested_rhat.nested_ref states the result bit for bit."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    M = int(chains_per_super)
    K = n_chains // M if M > 0 else 0
    want = dict(nrhat=want_nrhat, mean=want_mean, between=want_between, within=want_within, mcse_mean=want_mcse_mean)
    res = {k: (np.zeros(d) if w else None) for k, w in want.items()}
    res["super_mean"] = np.zeros((K, d)) if want_super_mean else None
    _check(lib().mi_mcmc_draw_stats_nested(_ptr(draws), mem, n_keep, d, n_chains, M, *[_ptr(res[k]) for k in
                                           ("nrhat", "mean", "between", "within", "mcse_mean", "super_mean")], stream or 0))
    return res


def draw_stats_nested_ranked(draws, chains_per_super, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, want_nrhat=True, want_nrhat_bulk=True,
                             want_nrhat_tail=True):
    """mi_mcmc_draw_stats_nested_ranked: the nested R-hat of the normal scores of x (nrhat_bulk) and of |x - median| (nrhat_tail), and the larger of
    the two (nrhat), per dimension of a slab as draw_stats_nested takes it; no split, so n_keep = 1 works.  Returns a dict of [d] arrays; an output that
    is not wanted is None.  mcmc_amd.nested_rhat.nested_ranked_ref states the result bit for bit."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    want = dict(nrhat=want_nrhat, nrhat_bulk=want_nrhat_bulk, nrhat_tail=want_nrhat_tail)
    res = {k: (np.zeros(d) if w else None) for k, w in want.items()}
    _check(lib().mi_mcmc_draw_stats_nested_ranked(_ptr(draws), mem, n_keep, d, n_chains, int(chains_per_super),
                                                  *[_ptr(res[k]) for k in ("nrhat", "nrhat_bulk", "nrhat_tail")], stream or 0))
    return res


def draws_order_stats(draws, ranks, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None):
    """mi_mcmc_draws_order_stats: out[a, i] = the value with the ranks[a]-th smallest key (0-based) among the n_keep * C pooled samples of
    dimension i of a slab [n_keep, d, C] (numpy array, or a device tensor / pointer with mem=MEM_DEVICE and explicit shape) -- exact; the order
    is that of mcmc_amd.quantiles.key.  Up to 32 ranks, unsorted or repeated.  Returns [len(ranks), d]."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    ranks = np.ascontiguousarray(ranks, dtype=np.uint64).ravel()
    out = np.zeros((ranks.size, d))
    _check(lib().mi_mcmc_draws_order_stats(_ptr(draws), mem, n_keep, d, n_chains,
                                           ranks.ctypes.data, ranks.size, out.ctypes.data, stream or 0))
    return out


def draws_quantiles(draws, probs, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None):
    """mi_mcmc_draws_quantiles: out[a, i] = the type-7 quantile (numpy's method="linear") at probs[a] of the pooled samples of dimension i,
    from two exact order statistics on the device (mcmc_amd.quantiles.quantiles_ref, bit for bit).  Up to 16 probabilities.  Returns
    [len(probs), d]."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    probs = np.ascontiguousarray(probs, dtype=np.float64).ravel()
    out = np.zeros((probs.size, d))
    _check(lib().mi_mcmc_draws_quantiles(_ptr(draws), mem, n_keep, d, n_chains,
                                         probs.ctypes.data, probs.size, out.ctypes.data, stream or 0))
    return out


def draws_to_chain_major_device(draws, n_keep, d, n_chains, out, stream=None):
    """mi_mcmc_draws_to_chain_major_device: slab [n_keep][d][C] in HBM -> [C][d][n_keep] in HBM (device tensors / pointers)."""
    _check(lib().mi_mcmc_draws_to_chain_major_device(_ptr(draws), n_keep, d, n_chains, _ptr(out), stream or 0))


def norm_ppf(p):
    """mi_mcmc_norm_ppf: the standard normal quantile as the library computes it on the host AND on the device (AS 241 PPND16 over the engine's
    deterministic logarithm; include/mi_mcmc.h).  Needs no device.  Returns an array of p's shape."""
    p = np.ascontiguousarray(p, dtype=np.float64)
    z = np.empty_like(p)
    _check(lib().mi_mcmc_norm_ppf(p.ctypes.data, p.size, z.ctypes.data))
    return z


def draws_rank_transform(draws, what="normal", split=False, fold=False, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, out=None):
    """mi_mcmc_draws_rank_transform: the exact average rank (what="average") or its normal score (what="normal") of every retained sample of a slab
    [n_keep, d, C] among the retained samples of its dimension (numpy array, or a device tensor / pointer with mem=MEM_DEVICE, explicit shape and a
    device `out`); split: the halves of every chain side by side, [n_keep // 2, d, 2 C]; fold: ranks of |x - median|.  mcmc_amd.rank_stats states
    the result bit for bit.  Returns the transformed slab (`out` where one was passed)."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    if what not in ("average", "normal", RANK_AVERAGE, RANK_NORMAL):
        raise ValueError(f"what = {what!r}: 'average' or 'normal'")
    w = {"average": RANK_AVERAGE, "normal": RANK_NORMAL}.get(what, what)
    flags = (RANK_SPLIT if split else 0) | (RANK_FOLD if fold else 0)
    if out is None:
        if mem != MEM_HOST:
            raise ValueError("a device slab needs a device `out`")
        out = np.zeros((n_keep // 2, d, 2 * n_chains) if split else (n_keep, d, n_chains))
    _check(lib().mi_mcmc_draws_rank_transform(_ptr(draws), mem, n_keep, d, n_chains, w, flags, _ptr(out), stream or 0))
    return out


def draw_stats_ranked(draws, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None):
    """mi_mcmc_draw_stats_ranked: rank-normalised split-R-hat (rhat = max(rhat_bulk, rhat_tail)), bulk-ESS and tail-ESS per dimension of a slab
    [n_keep, d, C] (Vehtari et al. 2021).  The ESS values are per half-chain: the many-chain figure is 2 C times them.  Returns a dict of [d] arrays."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    names = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")
    res = {k: np.zeros(d) for k in names}
    _check(lib().mi_mcmc_draw_stats_ranked(_ptr(draws), mem, n_keep, d, n_chains,
                                           *[res[k].ctypes.data for k in names], stream or 0))
    return res


def draw_stats_ranked_lags(draws, max_lag=None, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None):
    """mi_mcmc_draw_stats_ranked_lags: draw_stats_ranked with every lag of the half-chains up to K = min(max_lag, n_keep // 2 - 1) (max_lag=None: every
    lag) in the bulk-ESS and the tail-ESS.  Returns a dict of [d] arrays, with ended (uint8): 1 only where all three ESS sums ended."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    names = ("rhat", "rhat_bulk", "rhat_tail", "ess_bulk", "ess_tail")
    res = {k: np.zeros(d) for k in names}
    res["ended"] = np.zeros(d, dtype=np.uint8)
    ml = STATS_ALL_LAGS if max_lag is None else int(max_lag)
    _check(lib().mi_mcmc_draw_stats_ranked_lags(_ptr(draws), mem, n_keep, d, n_chains, ml,
                                                *[res[k].ctypes.data for k in names], res["ended"].ctypes.data, stream or 0))
    return res


def draws_log_kernel(target, draws, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, out=None):
    """mi_mcmc_draws_log_kernel: the log-posterior trace out[t, c] = log K(draws[t, :, c]) of a slab [n_keep, d, C] under `target` (make_target; d is
    the target's) -- numpy array, a 2-D [d, C] array being the case n_keep = 1, the chains' state; or a device tensor / pointer with mem=MEM_DEVICE,
    explicit n_keep and n_chains and a device `out`, written on `stream` without waiting.  include/mi_mcmc.h states the value bit for bit.  Returns
    [n_keep, C] (`out` where one was passed): as [n_keep, 1, C] it is a slab that draw_stats, draw_stats_ranked and draws_quantiles take."""
    d = int(target.d)
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 2:
            draws = draws[None]
        n_keep, d_slab, n_chains = draws.shape
        if d_slab != d:
            raise ValueError(f"the slab has d = {d_slab}, the target d = {d}")
    if out is None:
        if mem != MEM_HOST:
            raise ValueError("a device slab needs a device `out`")
        out = np.zeros((int(n_keep), int(n_chains)))
    _check(lib().mi_mcmc_draws_log_kernel(C.byref(target), _ptr(draws), mem, int(n_keep), int(n_chains), _ptr(out), stream or 0))
    return out


def test_logk_plan(kind, d, n_rows, n_keep, n_chains, slab_host=True, target_host=True):
    """mi_mcmc_test_logk_plan (TEST HOOK, mi_mcmc_probes.h): the plan of a draws_log_kernel call, host arithmetic -- a dict of route (0 one lane per column,
    1 the fused matrix product), grid, block, lds_bytes, Kp, ldA, n_row_tiles, ws_bytes."""
    o = (C.c_uint64 * 8)()
    lib().mi_mcmc_test_logk_plan(int(kind), int(d), int(n_rows), int(n_keep), int(n_chains),
                                 int(bool(slab_host)), int(bool(target_host)), o)
    return dict(zip(("route", "grid", "block", "lds_bytes", "Kp", "ldA", "n_row_tiles", "ws_bytes"), (int(v) for v in o)))


def draws_waic(target, draws, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, want_lppd=True, want_p_waic=True, want_loglik=False, want_summary=True,
               lppd=None, p_waic=None, loglik=None):
    """mi_mcmc_draws_waic: per observation r of `target` (make_target; LOGISTIC or NORMAL_MODEL) the log pointwise predictive density lppd[r] and the
    effective number of parameters p_waic[r] of a slab [n_keep, d, C], on request the pointwise log-likelihood loglik[r, t, c] itself, and
    summary = (elpd_waic, p_waic, lppd, se_elpd) -- numpy array, a 2-D [d, C] array being the case n_keep = 1; or a device tensor / pointer with
    mem=MEM_DEVICE, explicit n_keep and n_chains and device tensors `lppd`, `p_waic`, `loglik` for what is wanted of them (written on `stream`; the call
    waits only where the summary is wanted).  include/mi_mcmc.h states every value bit for bit, mcmc_amd.waic repeats it in numpy.  Returns a dict
    of lppd, p_waic, loglik ([n_rows, n_keep, C]: row r as [n_keep, 1, C] is a slab that draw_stats and draws_quantiles take) and summary (a dict);
    what was not asked for is None."""
    d, n_rows = int(target.d), int(target.n_rows)
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 2:
            draws = draws[None]
        n_keep, d_slab, n_chains = draws.shape
        if d_slab != d:
            raise ValueError(f"the slab has d = {d_slab}, the target d = {d}")
        lppd = np.zeros(n_rows) if want_lppd else None
        p_waic = np.zeros(n_rows) if want_p_waic else None
        loglik = np.zeros((n_rows, int(n_keep), int(n_chains))) if want_loglik else None
    summ = np.zeros(4) if want_summary else None
    _check(lib().mi_mcmc_draws_waic(C.byref(target), _ptr(draws), mem, int(n_keep), int(n_chains),
                                    _ptr(lppd), _ptr(p_waic), _ptr(loglik), _ptr(summ), stream or 0))
    summary = None if summ is None else dict(zip(("elpd_waic", "p_waic", "lppd", "se_elpd"), (float(v) for v in summ)))
    return dict(lppd=lppd, p_waic=p_waic, loglik=loglik, summary=summary)


def test_waic_plan(kind, d, n_rows, n_keep, n_chains, slab_host=True, target_host=True, want_loglik=False):
    """mi_mcmc_test_waic_plan (TEST HOOK, mi_mcmc_probes.h): the plan of a draws_waic call, host arithmetic -- a dict of route (0 elementwise, 1 the
    matrix product), chunk, n_chunks, grid, block, lds_bytes, ldR, Kp, merge_grid, ws_bytes."""
    o = (C.c_uint64 * 10)()
    lib().mi_mcmc_test_waic_plan(int(kind), int(d), int(n_rows), int(n_keep), int(n_chains),
                                 int(bool(slab_host)), int(bool(target_host)), int(bool(want_loglik)), o)
    return dict(zip(("route", "chunk", "n_chunks", "grid", "block", "lds_bytes", "ldR", "Kp", "merge_grid", "ws_bytes"), (int(v) for v in o)))


def draws_predict(target, draws, seed=0, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, want_p_mean=True, want_p_var=True, want_rep_freq=True,
                  want_prob=False, want_yrep=False, want_t_rep=True, want_ll_rep=True, want_ll_obs=None, want_summary=None,
                  p_mean=None, p_var=None, rep_freq=None, prob=None, yrep=None, t_rep=None, ll_rep=None, ll_obs=None):
    """mi_mcmc_draws_predict: posterior predictive checks of a slab [n_keep, d, C] under a LOGISTIC `target` (make_target; X are the rows to predict at --
    held-out data or a grid will do --, y may be None).  Per row r: p_mean[r], p_var[r], the posterior mean and variance of P(y = 1 | x_r), and rep_freq[r],
    the frequency of replicated successes; on request prob[r, t, c] and the replicates yrep[r, t, c] (0.0 / 1.0) drawn with `seed`.  Per draw: t_rep[t, c]
    (replicated successes), ll_rep[t, c] and, with y, ll_obs[t, c]; summary = (t_obs, ppp_t, ppp_dev, t_rep_mean), with y.  want_ll_obs / want_summary
    default to whether the target has y.  A numpy slab, a 2-D [d, C] array being the case n_keep = 1; or a device tensor / pointer with mem=MEM_DEVICE,
    explicit n_keep and n_chains and device tensors for what is wanted of the eight arrays (written on `stream`; the call waits only where the summary
    is wanted).  include/mi_mcmc.h states every value bit for bit, mcmc_amd.predict repeats it in numpy.  Returns a dict; what was not asked for is None."""
    d, n_rows = int(target.d), int(target.n_rows)
    has_y = bool(target.y)
    want_ll_obs = has_y if want_ll_obs is None else want_ll_obs
    want_summary = has_y if want_summary is None else want_summary
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 2:
            draws = draws[None]
        n_keep, d_slab, n_chains = draws.shape
        if d_slab != d:
            raise ValueError(f"the slab has d = {d_slab}, the target d = {d}")
        n, Cn = int(n_keep), int(n_chains)
        p_mean = np.zeros(n_rows) if want_p_mean else None
        p_var = np.zeros(n_rows) if want_p_var else None
        rep_freq = np.zeros(n_rows) if want_rep_freq else None
        prob = np.zeros((n_rows, n, Cn)) if want_prob else None
        yrep = np.zeros((n_rows, n, Cn)) if want_yrep else None
        t_rep = np.zeros((n, Cn)) if want_t_rep else None
        ll_rep = np.zeros((n, Cn)) if want_ll_rep else None
        ll_obs = np.zeros((n, Cn)) if want_ll_obs else None
    summ = np.zeros(4) if want_summary else None
    outs = (p_mean, p_var, rep_freq, prob, yrep, t_rep, ll_rep, ll_obs)
    _check(lib().mi_mcmc_draws_predict(C.byref(target), _ptr(draws), mem, int(n_keep), int(n_chains),
                                       int(seed), *[_ptr(o) for o in outs], _ptr(summ), stream or 0))
    summary = None if summ is None else dict(zip(("t_obs", "ppp_t", "ppp_dev", "t_rep_mean"), (float(v) for v in summ)))
    return dict(p_mean=p_mean, p_var=p_var, rep_freq=rep_freq, prob=prob, yrep=yrep, t_rep=t_rep, ll_rep=ll_rep, ll_obs=ll_obs, summary=summary)


def draws_psis_loo(target, draws, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, want_elpd_loo=True, want_pareto_k=True, want_lppd=True, want_summary=True,
                   elpd_loo=None, pareto_k=None, lppd=None):
    """mi_mcmc_draws_psis_loo: per observation r of `target` (make_target; LOGISTIC or NORMAL_MODEL) the PSIS-LOO estimate elpd_loo[r], the Pareto shape
    pareto_k[r] of its importance ratios and lppd[r] (mi_mcmc_draws_waic's, the same bits) of a slab [n_keep, d, C], and summary = (elpd_loo, p_loo, lppd,
    se_elpd_loo, n_bad: the rows with k > 0.7, NaN or inf) -- numpy array, a 2-D [d, C] array being the case n_keep = 1; or a device tensor / pointer with
    mem=MEM_DEVICE, explicit n_keep and n_chains and device tensors `elpd_loo`, `pareto_k`, `lppd` for what is wanted of them.  The call always waits.
    include/mi_mcmc.h states every value bit for bit, mcmc_amd.psis repeats it in numpy.  Returns a dict of elpd_loo, pareto_k, lppd ([n_rows]) and summary
    (a dict); what was not asked for is None."""
    d, n_rows = int(target.d), int(target.n_rows)
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        if draws.ndim == 2:
            draws = draws[None]
        n_keep, d_slab, n_chains = draws.shape
        if d_slab != d:
            raise ValueError(f"the slab has d = {d_slab}, the target d = {d}")
        elpd_loo = np.zeros(n_rows) if want_elpd_loo else None
        pareto_k = np.zeros(n_rows) if want_pareto_k else None
        lppd = np.zeros(n_rows) if want_lppd else None
    summ = np.zeros(5) if want_summary else None
    _check(lib().mi_mcmc_draws_psis_loo(C.byref(target), _ptr(draws), mem, int(n_keep), int(n_chains),
                                        _ptr(elpd_loo), _ptr(pareto_k), _ptr(lppd), _ptr(summ), stream or 0))
    summary = None if summ is None else dict(zip(("elpd_loo", "p_loo", "lppd", "se_elpd_loo", "n_bad"), (float(v) for v in summ)))
    return dict(elpd_loo=elpd_loo, pareto_k=pareto_k, lppd=lppd, summary=summary)


def test_set_psis_ll_bytes(n_bytes):
    """mi_mcmc_test_set_psis_ll_bytes (TEST HOOK, mi_mcmc_probes.h): the budget of a row group's block ll of draws_psis_loo (0 = the real one)."""
    lib().mi_mcmc_test_set_psis_ll_bytes(int(n_bytes))


def test_set_psis_lds_tail(n_doubles):
    """mi_mcmc_test_set_psis_lds_tail (TEST HOOK, mi_mcmc_probes.h): the tail values draws_psis_loo keeps in LDS (0 = the real capacity)."""
    lib().mi_mcmc_test_set_psis_lds_tail(int(n_doubles))


def test_psis_plan(kind, d, n_rows, n_keep, n_chains, slab_host=True, target_host=True):
    """mi_mcmc_test_psis_plan (TEST HOOK, mi_mcmc_probes.h): the plan of a draws_psis_loo call under the hooks set, host arithmetic -- a dict of M, m, G,
    n_groups, last_rows, tail_route (0 LDS, 1 re-read), lds_bytes, n_pieces, piece, sort_rows, ll_bytes, ws_bytes."""
    o = (C.c_uint64 * 12)()
    lib().mi_mcmc_test_psis_plan(int(kind), int(d), int(n_rows), int(n_keep), int(n_chains),
                                 int(bool(slab_host)), int(bool(target_host)), o)
    return dict(zip(("M", "m", "G", "n_groups", "last_rows", "tail_route", "lds_bytes", "n_pieces", "piece", "sort_rows", "ll_bytes", "ws_bytes"), (int(v) for v in o)))


def _loglik_shape(loglik, layout, n_rows, n_keep, n_chains, mem):
    if layout not in (LOGLIK_ROWS, LOGLIK_SLAB):
        raise ValueError(f"layout = {layout!r}: LOGLIK_ROWS or LOGLIK_SLAB")
    if mem == MEM_HOST:
        loglik = np.ascontiguousarray(loglik, dtype=np.float64)
        if loglik.ndim == 2:                              # [n_rows, K]: the case n_keep = 1
            loglik = loglik[:, None, :] if layout == LOGLIK_ROWS else loglik[None]
        if layout == LOGLIK_ROWS:
            n_rows, n_keep, n_chains = loglik.shape
        else:
            n_keep, n_rows, n_chains = loglik.shape
    return loglik, int(n_rows), int(n_keep), int(n_chains)


def loglik_waic(loglik, layout=LOGLIK_ROWS, n_rows=None, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, want_lppd=True, want_p_waic=True, want_summary=True,
                lppd=None, p_waic=None):
    """mi_mcmc_loglik_waic: draws_waic's lppd[r], p_waic[r] and summary of a pointwise log-likelihood matrix of the caller's own -- what a user-defined
    target has instead of a built-in one.  loglik: a numpy array [n_rows, n_keep, C] (layout=LOGLIK_ROWS, the layout of draws_waic's loglik; 2-D
    [n_rows, K] being n_keep = 1) or [n_keep, n_rows, C] (LOGLIK_SLAB, a draws slab whose dimensions are the observations); or a device tensor / pointer
    with mem=MEM_DEVICE, explicit n_rows, n_keep and n_chains and device tensors `lppd`, `p_waic` for what is wanted of them (written on `stream`; the call
    waits only where the summary is wanted).  The bits are those of mcmc_amd.waic.row_stats and summary.  Returns a dict of lppd, p_waic, loglik (always
    None: the matrix is the caller's) and summary (a dict); what was not asked for is None."""
    loglik, n_rows, n_keep, n_chains = _loglik_shape(loglik, layout, n_rows, n_keep, n_chains, mem)
    if mem == MEM_HOST:
        lppd = np.zeros(n_rows) if want_lppd else None
        p_waic = np.zeros(n_rows) if want_p_waic else None
    summ = np.zeros(4) if want_summary else None
    _check(lib().mi_mcmc_loglik_waic(_ptr(loglik), layout, mem, n_rows, n_keep, n_chains,
                                     _ptr(lppd), _ptr(p_waic), _ptr(summ), stream or 0))
    summary = None if summ is None else dict(zip(("elpd_waic", "p_waic", "lppd", "se_elpd"), (float(v) for v in summ)))
    return dict(lppd=lppd, p_waic=p_waic, loglik=None, summary=summary)


def loglik_psis_loo(loglik, layout=LOGLIK_ROWS, n_rows=None, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, want_elpd_loo=True, want_pareto_k=True,
                    want_lppd=True, want_summary=True, elpd_loo=None, pareto_k=None, lppd=None):
    """mi_mcmc_loglik_psis_loo: draws_psis_loo's elpd_loo[r], pareto_k[r], lppd[r] and summary of a pointwise log-likelihood matrix of the caller's own
    (loglik, layout and the device form as loglik_waic's; device tensors `elpd_loo`, `pareto_k`, `lppd`).  The call always waits.  The bits are those of
    mcmc_amd.psis.psis_ref.  Returns a dict of elpd_loo, pareto_k, lppd ([n_rows]) and summary (a dict); what was not asked for is None."""
    loglik, n_rows, n_keep, n_chains = _loglik_shape(loglik, layout, n_rows, n_keep, n_chains, mem)
    if mem == MEM_HOST:
        elpd_loo = np.zeros(n_rows) if want_elpd_loo else None
        pareto_k = np.zeros(n_rows) if want_pareto_k else None
        lppd = np.zeros(n_rows) if want_lppd else None
    summ = np.zeros(5) if want_summary else None
    _check(lib().mi_mcmc_loglik_psis_loo(_ptr(loglik), layout, mem, n_rows, n_keep, n_chains,
                                         _ptr(elpd_loo), _ptr(pareto_k), _ptr(lppd), _ptr(summ), stream or 0))
    summary = None if summ is None else dict(zip(("elpd_loo", "p_loo", "lppd", "se_elpd_loo", "n_bad"), (float(v) for v in summ)))
    return dict(elpd_loo=elpd_loo, pareto_k=pareto_k, lppd=lppd, summary=summary)


def test_loglik_plan(layout, n_rows, n_keep, n_chains, mat_host=True, psis=True):
    """mi_mcmc_test_loglik_plan (TEST HOOK, mi_mcmc_probes.h): the plan of a loglik_waic (psis=False) or loglik_psis_loo call under the hooks set, host
    arithmetic -- a dict of n_chunks, fold_grid, M, m, sort_rows, sort_groups, tail_route (0 LDS, 1 re-read), ws_bytes."""
    o = (C.c_uint64 * 8)()
    lib().mi_mcmc_test_loglik_plan(int(layout), int(n_rows), int(n_keep), int(n_chains),
                                   int(bool(mat_host)), int(bool(psis)), o)
    return dict(zip(("n_chunks", "fold_grid", "M", "m", "sort_rows", "sort_groups", "tail_route", "ws_bytes"), (int(v) for v in o)))


BRIDGE_SUMMARY = ("logml", "status", "it", "rel", "lstar", "cv1", "cv2", "n_prop")


def _bridge_summary(summ):
    return None if summ is None else dict(zip(BRIDGE_SUMMARY, (float(v) for v in summ)))


def bridge_proposal(draws, n_fit=0, n_prop=0, seed=0, n_keep=None, d=None, n_chains=None, mem=MEM_HOST, stream=None, want_prop=True, want_logg_post=True,
                    want_logg_prop=True, want_mean=True, want_cov=True, prop=None, logg_post=None, logg_prop=None):
    """mi_mcmc_bridge_proposal: the Gaussian proposal of bridge sampling, fitted to rows t < n_fit (0: n_keep // 2) of a slab [n_keep, d, C] -- n_prop (0: as
    many as the iteration part has samples) draws of it (prop [1, d, N2]), its log-density at the iteration part (logg_post [n_it, C]) and at its own draws
    (logg_prop [N2]), the fitted mean and cov, status (1: the fit is singular or not finite, every other output NaN) and ldh.  A numpy slab, or a device
    tensor / pointer with mem=MEM_DEVICE, explicit shape and device tensors `prop`, `logg_post`, `logg_prop` for what is wanted of them.  The call always
    waits.  include/mi_mcmc.h states every value bit for bit, mcmc_amd.bridge repeats it in numpy.  A target of the caller's own evaluates its log-kernel on
    prop and on the iteration part and hands the four arrays to bridge_estimate.  Returns a dict; what was not asked for is None."""
    draws, n_keep, d, n_chains = _slab_shape(draws, n_keep, d, n_chains, mem)
    nf = int(n_fit) if n_fit else n_keep // 2
    n_it = n_keep - nf
    N2 = int(n_prop) if n_prop else n_it * n_chains
    if mem == MEM_HOST:
        prop = np.zeros((1, d, N2)) if want_prop else None
        logg_post = np.zeros((max(n_it, 0), n_chains)) if want_logg_post else None
        logg_prop = np.zeros(N2) if want_logg_prop else None
    mean = np.zeros(d) if want_mean else None
    cov = np.zeros((d, d)) if want_cov else None
    info = np.zeros(2)
    _check(lib().mi_mcmc_bridge_proposal(_ptr(draws), mem, n_keep, d, n_chains, int(n_fit),
                                         int(n_prop), int(seed), _ptr(prop), _ptr(logg_post), _ptr(logg_prop),
                                         _ptr(mean), _ptr(cov), info.ctypes.data, stream or 0))
    return dict(prop=prop, logg_post=logg_post, logg_prop=logg_prop, mean=mean, cov=cov, status=int(info[0]), ldh=float(info[1]))


def bridge_estimate(logp_post, logg_post, logp_prop, logg_prop, n_it=None, n_chains=None, n_prop=0, n_eff=0.0, tol=0.0, max_iter=0, mem=MEM_HOST, stream=None,
                    want_f2=True, f2=None):
    """mi_mcmc_bridge_estimate: the iterative bridge-sampling estimate of the log marginal likelihood from the target's log-kernel (logp) and the proposal's
    log-density (logg) at the iteration part ([n_it, C]) and at the proposal draws ([N2]) -- numpy arrays, or device tensors / pointers with mem=MEM_DEVICE,
    explicit n_it, n_chains and n_prop and a device `f2` where wanted.  n_eff 0: N1; tol 0: 1e-10; max_iter 0: 1000.  The call always waits.  Returns a dict
    of f2 ([n_it, C]: as [n_it, 1, C] a slab that draw_stats takes) and summary (a dict of logml, status -- 0 converged, 2 max_iter, 3 r not positive and
    finite --, it, rel, lstar, cv1, cv2, n_prop); the relative mean-squared error of the estimate is cv1 + (n_it / ESS) * cv2 with draw_stats' ESS of f2."""
    if mem == MEM_HOST:
        logp_post, logg_post = (np.ascontiguousarray(a, dtype=np.float64) for a in (logp_post, logg_post))
        logp_prop, logg_prop = (np.ascontiguousarray(a, dtype=np.float64).ravel() for a in (logp_prop, logg_prop))
        if logp_post.ndim != 2 or logg_post.shape != logp_post.shape or logg_prop.shape != logp_prop.shape:
            raise ValueError("logp_post and logg_post are [n_it, C], logp_prop and logg_prop [N2]")
        n_it, n_chains = logp_post.shape
        n_prop = logp_prop.size
        f2 = np.zeros((n_it, n_chains)) if want_f2 else None
    summ = np.zeros(8)
    _check(lib().mi_mcmc_bridge_estimate(_ptr(logp_post), _ptr(logg_post), _ptr(logp_prop), _ptr(logg_prop), mem,
                                         int(n_it), int(n_chains), int(n_prop), float(n_eff), float(tol),
                                         int(max_iter), _ptr(f2), summ.ctypes.data, stream or 0))
    return dict(f2=f2, summary=_bridge_summary(summ))


def draws_bridge(target, draws, n_fit=0, n_prop=0, seed=0, n_eff=0.0, tol=0.0, max_iter=0, n_keep=None, n_chains=None, mem=MEM_HOST, stream=None, want_f2=True,
                 want_mean=True, want_cov=True, f2=None):
    """mi_mcmc_draws_bridge: the log marginal likelihood log of the integral of the target's kernel by bridge sampling with a Gaussian proposal, from a slab
    [n_keep, d, C] of posterior draws under `target` (make_target: ISO, DIAG, DENSE or LOGISTIC), on the device -- bridge_proposal, draws_log_kernel on the
    iteration part and on the proposal draws, and bridge_estimate composed, the same bits.  A numpy slab, or a device tensor / pointer with mem=MEM_DEVICE,
    explicit n_keep and n_chains and a device `f2` where wanted.  Returns a dict of f2, mean, cov and summary (bridge_estimate's; status 1: the fit is
    singular or not finite)."""
    d = int(target.d)
    if mem == MEM_HOST:
        draws = np.ascontiguousarray(draws, dtype=np.float64)
        n_keep, d_slab, n_chains = draws.shape
        if d_slab != d:
            raise ValueError(f"the slab has d = {d_slab}, the target d = {d}")
        nf = int(n_fit) if n_fit else n_keep // 2
        f2 = np.zeros((max(n_keep - nf, 0), n_chains)) if want_f2 else None
    mean = np.zeros(d) if want_mean else None
    cov = np.zeros((d, d)) if want_cov else None
    summ = np.zeros(8)
    _check(lib().mi_mcmc_draws_bridge(C.byref(target), _ptr(draws), mem, int(n_keep), int(n_chains), int(n_fit),
                                      int(n_prop), int(seed), float(n_eff), float(tol), int(max_iter),
                                      _ptr(f2), _ptr(mean), _ptr(cov), summ.ctypes.data, stream or 0))
    return dict(f2=f2, mean=mean, cov=cov, summary=_bridge_summary(summ))


def test_set_bridge_prop_bytes(n_bytes):
    """mi_mcmc_test_set_bridge_prop_bytes (TEST HOOK, mi_mcmc_probes.h): the budget of one group of proposal columns of bridge sampling (0 = the real one)."""
    lib().mi_mcmc_test_set_bridge_prop_bytes(int(n_bytes))
