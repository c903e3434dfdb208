"""The route and the bits of the sampler entry points (hmc / mala / rwmh / nuts), one line per call, at the sizes where their routing ladders turn
(GPU box).  A call that succeeds prints last_kernel() and a SHA-256 (16 hex digits) of every output; a call the library refuses prints its return code
and message.  No assertion and no probe beyond last_kernel(), so it also runs on the library of another commit that MI_MCMC_LIB names: two runs, one
per library, whose outputs are the same in every line took the same routes and computed the same bits.
    python tools/sampler_route_bits.py > this.txt;  MI_MCMC_LIB=/path/to/other/libmi_mcmc.so python tools/sampler_route_bits.py > other.txt"""
import hashlib, os, sys
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import numpy as np
import torch
import mcmc_amd
from mcmc_amd import synth

C, N_BURNIN, N_KEEP, N_LEAP, DEPTH, N_ROWS = 40, 2, 3, 3, 3, 24      # 40 chains: no multiple of 16, more than one 32-slot group
ALGOS = ("hmc", "mala", "rwmh", "nuts")
ISO, DIAG, DENSE, LOGISTIC, NORMAL = (mcmc_amd.TARGET_GAUSS_ISO, mcmc_amd.TARGET_GAUSS_DIAG, mcmc_amd.TARGET_GAUSS_DENSE, mcmc_amd.TARGET_LOGISTIC,
                                      mcmc_amd.TARGET_NORMAL_MODEL)
KIND_NAME = {ISO: "iso", DIAG: "diag", DENSE: "dense", LOGISTIC: "logistic", NORMAL: "normal_model"}
dev = torch.device("cuda", 0)


def digest(a):
    if hasattr(a, "cpu"): a = a.cpu().numpy()
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def target_data(kind, d):
    """prec, X, y of a shape"""
    if kind == DIAG: return dict(prec=synth.ill_conditioned_diag(d, 50.0))
    if kind == DENSE: return dict(prec=synth.dense_gaussian_precision(d))
    if kind == LOGISTIC: X, y = synth.logistic_problem(d, N_ROWS); return dict(X=X, y=y)
    if kind == NORMAL: return dict(y=np.random.default_rng(8).normal(1.0, 2.0, N_ROWS))
    return {}


_init = {}
def initial(kind, d):
    if (kind, d) not in _init:
        x = np.clip(synth.initial_states(C, d, seed=9) * 0.3, -1.0, 1.0)
        if kind == NORMAL: x[:, 1] = np.abs(x[:, 1]) + 0.5      # (sigma)
        _init[(kind, d)] = x
    return _init[(kind, d)].copy()


def spd(d):
    A = np.random.default_rng(5).standard_normal((d, d)); return A @ A.T / d + np.eye(d)


def setting(name, d):
    """the six settings every shape is crossed with"""
    kw = {}
    if "bounds" in name:
        t = np.random.default_rng(1).integers(1, 5, d)          # determine_bounds_type: none, lower, upper, both
        kw.update(vals_bound=1, lower_bounds=np.where((t == 2) | (t == 4), -1.5, -np.inf), upper_bounds=np.where((t == 3) | (t == 4), 2.0, np.inf))
    if "diag" in name: kw["precond_mat"] = np.diag(np.random.default_rng(3).uniform(0.5, 2.0, d))
    if "dense" in name: kw["precond_mat"] = spd(d)
    return kw
SETTINGS = ("plain", "diag", "dense", "bounds", "bounds+diag", "bounds+dense")


def call(name, algo, kind, d, init=None, mem=mcmc_amd.MEM_HOST, hint=mcmc_amd.KERNEL_AUTO, data=None, mass_diag=None, draw0=0, step_in=None, adapt_in=None,
         n_burnin=N_BURNIN, n_keep=N_KEEP, **skw):
    skw.setdefault("max_tree_depth", DEPTH)
    st = mcmc_amd.default_settings(rng_seed_value=11, n_burnin_draws=n_burnin, n_keep_draws=n_keep, n_leap_steps=N_LEAP, n_adapt_draws=4,
                                   step_size=0.3 if algo == "nuts" else 0.05, **skw)
    init = initial(kind, d) if init is None else init
    data = target_data(kind, d) if data is None else data
    n_alloc = min(n_keep, 16)                              # (the argument-error cases ask for draws nobody allocates: they fail before any is written)
    n_tot = min(n_burnin, 16) + n_alloc
    nuts = algo == "nuts"
    host = dict(theta=np.array(init.T, order="C", copy=True), draws=np.zeros((n_alloc, d, C)), n_accept=np.zeros(C, dtype=np.uint64),
                n_leap=np.zeros(C, dtype=np.uint64), n_exec=np.zeros(C, dtype=np.uint64))
    if nuts:
        host.update(eps=np.zeros(C) if step_in is None else np.array(step_in, copy=True), depth=np.zeros((n_tot, C), dtype=np.uint32),
                    adapt_state=np.zeros((3, C)) if adapt_in is None else np.array(adapt_in, copy=True))
    if mass_diag is not None: mass_diag = np.ascontiguousarray(mass_diag)
    if mem == mcmc_amd.MEM_DEVICE:
        up = lambda a: None if a is None else torch.from_numpy(a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a).to(dev)
        data = {k: up(np.ascontiguousarray(v, dtype=np.float64)) for k, v in data.items()}
        out = {k: up(v) for k, v in host.items()}
        mass_diag = up(mass_diag)
        torch.cuda.synchronize()
    else: out = host
    t = mcmc_amd.make_target(kind, d, mem=mem, kernel_hint=hint, **data)
    ch = mcmc_amd.make_chains(out["theta"], C, draws=out["draws"], n_accept=out["n_accept"], n_leapfrogs=out["n_leap"], n_leapfrogs_executed=out["n_exec"],
                              step_size=out.get("eps"), nuts_depth=out.get("depth"), nuts_adapt_state=out.get("adapt_state"), mem=mem, draw0=draw0,
                              mass_diag=mass_diag)
    try:
        mcmc_amd.run(algo, t, st, ch)
        torch.cuda.synchronize()
    except mcmc_amd.MiMcmcError as e:
        print(f"{name:72s} rc {e.code} {mcmc_amd.lib().mi_mcmc_last_error().decode()}", flush=True)
        return None
    print(f"{name:72s} {mcmc_amd.last_kernel()} | " + " ".join(f"{k} {digest(v)}" for k, v in out.items()), flush=True)
    return out


SHAPES = [(k, d) for k in (ISO, DIAG, DENSE) for d in (4, 20, 70, 130, 520)] + [(LOGISTIC, d) for d in (4, 12, 130, 520)] + [(NORMAL, 2)]
for kind, d in SHAPES:
    for algo in ALGOS:
        for s in SETTINGS:
            call(f"{algo} {KIND_NAME[kind]} d={d} {s}", algo, kind, d, **setting(s, d))
            if s in ("plain", "diag", "bounds"):           # ... and with target and chains in device memory
                call(f"{algo} {KIND_NAME[kind]} d={d} {s} device", algo, kind, d, mem=mcmc_amd.MEM_DEVICE, **setting(s, d))

# kernel hints
H = mcmc_amd
for h in ("KERNEL_HMC_TWO_WAVES_PER_SIMD", "KERNEL_HMC_ONE_WAVE_PER_SIMD", "KERNEL_HMC_SPLIT2", "KERNEL_HMC_SPLIT4", "KERNEL_HMC_SPLIT4_TWO_WAVES"):
    call(f"hmc dense d=70 {h}", "hmc", DENSE, 70, hint=getattr(H, h))
for h in ("KERNEL_ELEMENTWISE_1LANE", "KERNEL_ELEMENTWISE_4LANE"):
    for kind, d in ((ISO, 20), (DIAG, 70), (DIAG, 130)):
        call(f"hmc {KIND_NAME[kind]} d={d} {h}", "hmc", kind, d, hint=getattr(H, h))
for kind, d in ((DENSE, 20), (DENSE, 130), (DENSE, 520), (LOGISTIC, 12), (LOGISTIC, 130), (ISO, 130)):
    for algo in ALGOS:
        for s in ("plain", "bounds+diag"):
            call(f"{algo} {KIND_NAME[kind]} d={d} {s} KERNEL_LITERAL", algo, kind, d, hint=H.KERNEL_LITERAL, **setting(s, d))
for h in ("KERNEL_NUTS_LOCKSTEP", "KERNEL_NUTS_TICK_LOCAL", "KERNEL_NUTS_MEMO_INTICK"):
    for s in ("plain", "diag", "bounds"):
        call(f"nuts dense d=20 {s} {h}", "nuts", DENSE, 20, hint=getattr(H, h), **setting(s, 20))

# per-chain diagonal masses (hmc)
for kind, d in ((ISO, 4), (DENSE, 20), (DENSE, 130)):
    mass = np.random.default_rng(6).uniform(0.5, 2.0, (d, C))
    for s in ("plain", "bounds"):
        call(f"hmc {KIND_NAME[kind]} d={d} {s} mass_diag", "hmc", kind, d, mass_diag=mass, **setting(s, d))
    call(f"hmc {KIND_NAME[kind]} d={d} plain mass_diag device", "hmc", kind, d, mass_diag=mass, mem=mcmc_amd.MEM_DEVICE)
call("mala dense d=20 mass_diag", "mala", DENSE, 20, mass_diag=np.ones((20, C)))
call("hmc dense d=20 mass_diag + precond_mat", "hmc", DENSE, 20, mass_diag=np.ones((20, C)), **setting("diag", 20))

# a nuts continuation that resumes after 2 draws inside the adaptation window (n_adapt_draws = 4)
for kind, d in ((DENSE, 20), (DENSE, 130), (DENSE, 520), (LOGISTIC, 4), (LOGISTIC, 130)):
    for s in ("plain", "diag"):
        first = call(f"nuts {KIND_NAME[kind]} d={d} {s} first 2 draws", "nuts", kind, d, n_burnin=2, n_keep=0, **setting(s, d))
        if first is None: continue
        call(f"nuts {KIND_NAME[kind]} d={d} {s} resumed at draw 2", "nuts", kind, d, init=np.ascontiguousarray(first["theta"].T), draw0=2, step_in=first["eps"],
             adapt_in=first["adapt_state"], n_burnin=0, n_keep=3, **setting(s, d))
call("nuts dense d=20 resumed without step sizes", "nuts", DENSE, 20, draw0=2)

# starts that send chains into the non-finite replay (the poisoned rows of tests/test_gpu_nonfinite.py), one per route family
def poisoned(kind, d):
    x = synth.initial_states(C, d, seed=9)
    x[3] *= 1.0e300; x[20, min(5, d - 1)] = -np.inf; x[37, d - 1] = np.nan; x[30] *= 1.0e160
    return x
for kind, d in ((DENSE, 20), (DENSE, 70), (DIAG, 130), (DENSE, 130), (DENSE, 520), (LOGISTIC, 130), (LOGISTIC, 520)):
    for algo in ALGOS:
        for s in ("plain", "diag"):
            call(f"{algo} {KIND_NAME[kind]} d={d} {s} non-finite start", algo, kind, d, init=poisoned(kind, d), **setting(s, d))
call("hmc dense d=20 mass_diag non-finite start", "hmc", DENSE, 20, init=poisoned(DENSE, 20), mass_diag=np.random.default_rng(6).uniform(0.5, 2.0, (20, C)))
call("hmc iso d=130 mass_diag non-finite start", "hmc", ISO, 130, init=poisoned(ISO, 130), mass_diag=np.random.default_rng(6).uniform(0.5, 2.0, (130, C)))

# argument errors: which check answers first is part of the record
for kind, d in SHAPES:
    for algo in ALGOS:
        tag = f"{algo} {KIND_NAME[kind]} d={d}"
        if kind == LOGISTIC:
            X, y = synth.logistic_problem(d, N_ROWS)
            call(f"{tag} no X", algo, kind, d, data=dict(y=y))
            call(f"{tag} no X, bounds", algo, kind, d, data=dict(y=y), **setting("bounds", d))
        if kind in (DIAG, DENSE): call(f"{tag} no prec", algo, kind, d, data={})
        call(f"{tag} vals_bound without bounds", algo, kind, d, vals_bound=1)
        call(f"{tag} vals_bound without bounds, diag", algo, kind, d, vals_bound=1, **setting("diag", d))
        call(f"{tag} 2^32 burn-in draws", algo, kind, d, n_burnin=2 ** 32, n_keep=0)
        call(f"{tag} 2^32 burn-in draws, vals_bound without bounds", algo, kind, d, n_burnin=2 ** 32, n_keep=0, vals_bound=1)
        call(f"{tag} 2^32 burn-in draws, bounds+diag", algo, kind, d, n_burnin=2 ** 32, n_keep=0, **setting("bounds+diag", d))
        if algo == "nuts":
            for depth in (11, 31):
                call(f"{tag} max_tree_depth {depth}", algo, kind, d, n_burnin=1, n_keep=1, max_tree_depth=depth)
                call(f"{tag} max_tree_depth {depth} diag", algo, kind, d, n_burnin=1, n_keep=1, max_tree_depth=depth, **setting("diag", d))
