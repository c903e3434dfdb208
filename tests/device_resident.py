"""Device-resident chains on a caller's stream: what bench.py, mcmc_amd.dist and production callers do, and mcmc_amd.sample() never does
(helper of tests/test_gpu_device_resident_routes.py and tests/test_gpu_mass_adapt_device.py; not collected).

A call is prepared, queued and collected:
  prepare  every output lives inside a longer tensor with GUARD elements before and after it, all of it filled with a sentinel; every device input
           (theta, the target's prec / X / y, mass_diag, the continuation's step_size / nuts_adapt_state) starts as the sentinel too.  The fills run
           on the default stream; the caller synchronises the device ONCE after the last prepare and before the first enqueue.
  enqueue  on the caller's (non-blocking) stream: some matrix products that take a while, then the non-blocking copies of the real input values, then
           the library call.  A read of the library that is not ordered behind the stream sees the sentinel, not the values.
  collect  after stream.synchronize() alone: the outputs as numpy, whether every guard still holds the sentinel, which outputs still hold one inside."""
import numpy as np
import torch

import mcmc_amd

GUARD = 64
F64_SENTINEL = 0x7FF8A5A5A5A5A5A5          # a NaN
U64_SENTINEL = 0xA5A5A5A5A5A5A5A5
U32_SENTINEL = 0xA5A5A5A5
_F64, _U64, _U32 = "f64", "u64", "u32"
_BITS = {_F64: (torch.int64, np.uint64, F64_SENTINEL), _U64: (torch.int64, np.uint64, U64_SENTINEL), _U32: (torch.int32, np.uint32, U32_SENTINEL)}


def _signed(bits, np_unsigned):
    return int(np.array([bits], dtype=np_unsigned).view(np.int64 if np_unsigned is np.uint64 else np.int32)[0])


class Guarded:
    """n elements of `kind` between two guards, every element the sentinel"""

    def __init__(self, kind, shape, dev):
        self.kind, self.shape, self.n = kind, tuple(shape), int(np.prod(shape, dtype=np.int64))
        tdt, self.np_unsigned, self.bits = _BITS[kind]
        self.raw = torch.full((self.n + 2 * GUARD,), _signed(self.bits, self.np_unsigned), dtype=tdt, device=dev)
        self.inner = self.raw[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return self.inner.data_ptr()

    def values(self):
        """the inner elements as a device tensor of the output's type (float64 / the raw signed integers)"""
        return self.inner.view(torch.float64) if self.kind == _F64 else self.inner

    def _host_bits(self):
        return self.raw.cpu().numpy().view(self.np_unsigned)

    def collect(self):
        b = self._host_bits()
        inner = b[GUARD:GUARD + self.n]
        guards_ok = bool((b[:GUARD] == self.bits).all() and (b[GUARD + self.n:] == self.bits).all())
        out = (inner.view(np.float64) if self.kind == _F64 else inner).reshape(self.shape).copy()
        return out, guards_ok, bool((inner == self.bits).any()), bool((inner == self.bits).all())


_busy = {}


def _busy_work(dev, rounds=6):
    """matrix products that keep the current stream busy for some milliseconds"""
    if dev not in _busy:
        a = torch.rand((3072, 3072), dtype=torch.float64, device=dev)
        _busy[dev] = (a, torch.empty_like(a))
    a, out = _busy[dev]
    for _ in range(rounds):
        torch.mm(a, a, out=out)


class Call:
    """One library call in device memory.  algo: "hmc" | "mala" | "rwmh" | "nuts" | "rmhmc" for mcmc_amd.run, or `call`: a function
    (target, settings, chains, stream_ptr, extra) -> anything, for the other entry points (its result is kept as .returned; `extra`: name -> Guarded, made from
    extra_outputs: name -> (kind, shape)).  outputs: the optional outputs the call passes (None: all of them); theta is always there."""
    ALL = ("draws", "n_accept", "step_size", "n_leapfrogs", "n_leapfrogs_executed", "nuts_depth", "nuts_adapt_state")

    def __init__(self, algo, kind, init, settings, prec=None, X=None, y=None, chain0=0, draw0=0, kernel_hint=mcmc_amd.KERNEL_AUTO, mass_diag=None,
                 step_size_in=None, adapt_state_in=None, outputs=None, call=None, extra_outputs=None, device=None):
        self.dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
        self.algo, self.kind, self.settings, self.call = algo, kind, settings, call
        init = np.ascontiguousarray(init, dtype=np.float64)
        self.C, self.d = init.shape
        C, d = self.C, self.d
        n_keep, n_tot = int(settings.n_keep_draws), int(settings.n_burnin_draws) + int(settings.n_keep_draws)
        want = set(self.ALL if outputs is None else outputs)
        if algo != "nuts":
            want -= {"nuts_depth", "nuts_adapt_state"}
        assert want <= set(self.ALL)
        shapes = dict(draws=(_F64, (n_keep, d, C)), n_accept=(_U64, (C,)), step_size=(_F64, (C,)), n_leapfrogs=(_U64, (C,)),
                      n_leapfrogs_executed=(_U64, (C,)), nuts_depth=(_U32, (n_tot, C)), nuts_adapt_state=(_F64, (3, C)))
        self.out = {"theta": Guarded(_F64, (d, C), self.dev)}
        for name in self.ALL:
            if name in want:
                self.out[name] = Guarded(*shapes[name], self.dev)
        self.extra = {k: Guarded(kd, shp, self.dev) for k, (kd, shp) in (extra_outputs or {}).items()}
        # device inputs: sentinel now, the values on the caller's stream
        self._copies, self._pinned = [], []
        self._produce(self.out["theta"].values(), init.T)
        self.t_in = {}
        for name, a in (("prec", prec), ("X", X), ("y", y)):
            self.t_in[name] = None if a is None else self._input(a)
        self.n_rows = 0 if X is None else int(np.shape(X)[0])
        self.mass_diag = None if mass_diag is None else self._input(np.asarray(mass_diag, dtype=np.float64).reshape(d, C))
        if step_size_in is not None:
            self._produce(self.out["step_size"].values(), step_size_in)
        if adapt_state_in is not None:
            self._produce(self.out["nuts_adapt_state"].values(), adapt_state_in)
        self.kernel_hint, self.chain0, self.draw0 = kernel_hint, int(chain0), int(draw0)
        self.kernel, self.returned = None, None

    def _input(self, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        t = torch.full((a.size,), _signed(F64_SENTINEL, np.uint64), dtype=torch.int64, device=self.dev).view(torch.float64)
        self._produce(t, a)
        return t

    def _produce(self, dst, values):
        src = torch.from_numpy(np.ascontiguousarray(values, dtype=np.float64).reshape(-1).copy()).pin_memory()
        assert src.numel() == dst.numel()
        self._pinned.append(src)
        self._copies.append((dst, src))

    def enqueue(self, stream):
        """on `stream` (a torch.cuda.Stream): the busy work, the inputs, the call"""
        o = self.out
        p = lambda name: o[name].ptr if name in o else None
        with torch.cuda.stream(stream):
            _busy_work(self.dev)
            for dst, src in self._copies:
                dst.copy_(src, non_blocking=True)
            t = mcmc_amd.make_target(self.kind, self.d, prec=self.t_in["prec"], X=self.t_in["X"], y=self.t_in["y"], mem=mcmc_amd.MEM_DEVICE,
                                     kernel_hint=self.kernel_hint)
            if self.t_in["X"] is not None:
                t.n_rows = self.n_rows                      # (make_target reads X.shape[0]; the inputs here are flat)
            c = mcmc_amd.make_chains(p("theta"), self.C, chain0=self.chain0, draws=p("draws"), n_accept=p("n_accept"), step_size=p("step_size"),
                                     n_leapfrogs=p("n_leapfrogs"), nuts_depth=p("nuts_depth"), mem=mcmc_amd.MEM_DEVICE, draw0=self.draw0,
                                     mass_diag=self.mass_diag, nuts_adapt_state=p("nuts_adapt_state"), n_leapfrogs_executed=p("n_leapfrogs_executed"))
            if self.call is not None:
                self.returned = self.call(t, self.settings, c, stream.cuda_stream, self.extra)
            else:
                mcmc_amd.run(self.algo, t, self.settings, c, stream=stream.cuda_stream)
            self.kernel = mcmc_amd.last_kernel()
        return self

    def collect(self):
        """after the stream is idle: a dict in mcmc_amd.sample()'s names (absent outputs: None) plus kernel, guards_ok, sentinel_left (the outputs
        that still hold a sentinel somewhere inside), untouched (the outputs that hold nothing else), returned and the extra outputs by their names"""
        names = dict(theta="theta", draws="draws", n_accept="n_accept", step_size="eps", n_leapfrogs="n_leap", n_leapfrogs_executed="n_exec",
                     nuts_depth="depth", nuts_adapt_state="adapt_state")
        r = {v: None for v in names.values()}
        r.update(kernel=self.kernel, returned=self.returned, guards_ok=True, sentinel_left=set(), untouched=set())
        for name, g in list(self.out.items()) + list(self.extra.items()):
            val, ok, some, every = g.collect()
            r[names.get(name, name)] = val
            r["guards_ok"] = r["guards_ok"] and ok
            if some:
                r["sentinel_left"].add(name)
            if every:
                r["untouched"].add(name)
        return r


def run_case(stream, *args, **kw):
    """prepare, synchronise the device once, queue on `stream`, wait for `stream` alone, collect"""
    call = Call(*args, **kw)
    torch.cuda.synchronize()
    call.enqueue(stream)
    stream.synchronize()
    return call.collect()
