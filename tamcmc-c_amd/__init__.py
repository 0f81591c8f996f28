"""tamcmc-c_amd: MI355X-native hot path of the TAMCMC parallel-tempered sampler.

Python here is plumbing only: a ctypes binding of the C ABI declared in
include/tamcmc_hip.h (built in-tree into libtamcmc_hip.so by `make`), used by the
tests, bench.py and __graft_entry__.  The compute path is the HIP library; there is
no CPU fallback -- a missing library or a missing GPU raises.

The directory name contains a hyphen, so import it through `load_package()` of
__graft_entry__.py (it registers this package as module `tamcmc_c_amd`).
"""
import ctypes as C
import weakref
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libtamcmc_hip.so")

OK = 0
ERR_HIP, ERR_EMPTY_WINDOW, ERR_NAN_WINDOW, ERR_BAD_MODEL, ERR_BAD_ARG, ERR_NO_SPECTRUM, ERR_NO_DEVICE = -1, -2, -3, -4, -5, -6, -7
MODEL_MS_GLOBAL_A1ETAA3_CLASSIC, MODEL_MS_LOCAL_BASIC, MODEL_MS_GLOBAL_AJ = 3, 11, 23
# height-per-m models (no inclination; include/tamcmc_hip.h): nine ratios shared by all orders / one height per (n, l, |m|), global
# (model level only) / the same for a local fit
MODEL_MS_GLOBAL_A1ETAA3_CLASSIC_V2, MODEL_MS_GLOBAL_A1ETAA3_CLASSIC_V3, MODEL_MS_LOCAL_HNLM = 12, 13, 14
MODEL_RGB_ASYMPT_AJ_CTEWIDTH_V4 = 27   # constant-width variant of 25, same path
MODEL_RGB_ASYMPT_AJ_APPWIDTH_V4 = 25  # batched device paths only (loglike_params_batch, fd_gradient*): needs the ARMM pre-step
PRECISION_STRICT, PRECISION_FAST, PRECISION_FAST_DIRECT = 0, 1, 2
OPT_PRECISION, OPT_TIMING, OPT_BINS_PER_THREAD, OPT_WORKGROUP, OPT_FD_WINDOWED, OPT_STEP_SCHEME, OPT_ARMM_DENSE_SCAN = 1, 2, 3, 4, 5, 6, 7
OPT_GRADIENT, GRADIENT_FD, GRADIENT_ADJOINT = 9, 0, 1  # gradient batches: finite differences (default) / table-space adjoint, frozen windows
OPT_RGB_DEVICE_LANGEVIN = 11  # 1: Sampler(use_drift=1, engine="device") is built for the red-giant ids 25 / 27 (default 0: ERR_BAD_MODEL); read at creation
OPT_ENVELOPE_DEVICE_ENGINE = 13  # 1: Sampler(engine="device", use_drift=0) is built for the Gaussian-envelope ids 0 / 1 (default 0: ERR_BAD_MODEL); read at creation
OPT_FACTOR_REFRESH = 14  # R: 0 / 1 a full factorisation in every adapting iteration (default); 2 ... 65536 rank-one steps of the proposal factor, a full one every R-th; read at creation
OPT_ENVELOPE_DEVICE_LANGEVIN = 17  # 1: Sampler(engine="device", use_drift=1) is built for the Gaussian-envelope ids 0 / 1 (default 0: ERR_BAD_MODEL); independent of option 13; read at creation
OPT_ENVELOPE_GRADIENT = 15  # 1: fd_gradient / fd_gradient_posterior (and the host engine's Langevin step) take the analytic likelihood share for ids 0 / 1 (default 0: brute force); read at every call
ENVELOPE_GRAD_N, ENVELOPE_KSI_N = 13, 9  # row quantities / xi sums per vector of HipContext.envelope_gradient_sums
OPT_RGB_ADJOINT = 12  # 1: under GRADIENT_ADJOINT the red-giant ids 25 / 27 take the hybrid adjoint batch (default 0: ERR_BAD_MODEL); read at every call
OPT_RGB_FISHER = 16  # 1: HipContext.fisher (and Sampler.seed_proposal_fisher) accepts the red-giant ids 25 / 27 (default 0: ERR_BAD_MODEL); read at every call
OPT_FISHER_WORKSPACE_MB = 10  # MiB of model rows HipContext.fisher keeps on the device per pass (default 2048)
FISHER_SLAB = 2048  # bins per workgroup of the Gram kernel (TAMCMC_FISHER_SLAB)
OPT_QUICK_DECIDE = 8  # test facility: 1 = the fused step's decision shortcut always falls back to the exact evaluation


class Multiplet(C.Structure):
    """struct tamcmc_multiplet (include/tamcmc_hip.h), 152 bytes."""
    _fields_ = [("l", C.c_int32), ("i0", C.c_int32), ("i1", C.c_int32), ("flags", C.c_int32),
                ("fc", C.c_double), ("gamma", C.c_double), ("asym", C.c_double),
                ("nu", C.c_double * 7), ("hv", C.c_double * 7)]


MULT_DTYPE = np.dtype([("l", "<i4"), ("i0", "<i4"), ("i1", "<i4"), ("flags", "<i4"), ("fc", "<f8"), ("gamma", "<f8"),
                       ("asym", "<f8"), ("nu", "<f8", (7,)), ("hv", "<f8", (7,))])
assert MULT_DTYPE.itemsize == 152 and C.sizeof(Multiplet) == 152

_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int32)
_vp = C.c_void_p

# every symbol include/tamcmc_hip.h declares: (name, restype, argtypes)
ABI = [
    ("tamcmc_hip_version", C.c_char_p, []),
    ("tamcmc_hip_create", C.c_int, [C.POINTER(_vp), C.c_int]),
    ("tamcmc_hip_destroy", None, [_vp]),
    ("tamcmc_hip_last_error", C.c_char_p, [_vp]),
    ("tamcmc_hip_set_option", C.c_int, [_vp, C.c_int, C.c_int64]),
    ("tamcmc_hip_host_alloc", C.c_void_p, [C.c_size_t]),
    ("tamcmc_hip_host_free", None, [_vp]),
    ("tamcmc_hip_set_spectrum", C.c_int, [_vp, _dp, _dp, C.c_int64]),
    ("tamcmc_hip_loglike_batch", C.c_int, [_vp, C.c_int, _vp, _ip, _dp, C.c_int, _ip, _ip, _dp, C.c_double, _dp, _dp]),
    ("tamcmc_build_mode_table", C.c_int, [C.c_int, _dp, _ip, _dp, C.c_int64, _vp, C.c_int, C.POINTER(C.c_int), _dp,
                                          C.POINTER(C.c_int), C.POINTER(C.c_int)]),
    ("tamcmc_hip_loglike_params_batch", C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int64, _ip, _dp, C.c_double, _dp, _dp, _ip]),
    ("tamcmc_hip_fd_gradient", C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int64, _ip, _ip, C.c_int, _dp, _dp, C.c_double, _dp, _dp]),
    ("tamcmc_hip_fd_gradient_posterior", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, C.c_int64, _ip, _ip, C.c_int, _dp, _dp, C.c_double,
                                                  _dp, _ip, _dp, _dp, _dp, _dp, _dp]),
    ("tamcmc_hip_adjoint_table", C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int64, _ip, _dp, C.c_double, _dp, _dp, C.POINTER(C.c_int)]),
    ("tamcmc_hip_envelope_gradient_sums", C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int64, _dp, _dp, _dp]),
    ("tamcmc_hip_fisher", C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int64, _ip, _ip, C.c_int, _dp, _dp, C.c_double, _dp]),
    ("tamcmc_hip_weighted_gram", C.c_int, [_vp, C.c_int, C.c_int64, _dp, _dp, _dp]),
    ("tamcmc_hip_get_fisher_times", C.c_int, [_vp, _dp, _dp, _dp]),
    ("tamcmc_hip_get_rgb_fisher_stats", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("tamcmc_hip_rgb_mixed_modes", C.c_int, [_vp, C.c_int, _dp, C.c_int64, _ip, C.c_int, _dp, _dp, _dp, C.POINTER(C.c_int)]),
    ("tamcmc_hip_get_kernel_stats", C.c_int, [_vp, _dp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("tamcmc_hip_reset_kernel_stats", C.c_int, [_vp]),
    ("tamcmc_hip_get_fd_stats", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("tamcmc_hip_get_fd_full_tables", C.c_int, [_vp, C.POINTER(C.c_int64)]),
    ("tamcmc_hip_rgb_batch_tables", C.c_int, [_vp, C.c_int, C.c_int, _dp, C.c_int64, _ip, _ip, C.c_int, _dp, _vp, _ip, _dp, _ip, _ip, _ip,
                                             C.POINTER(C.c_int)]),
    ("tamcmc_hip_fd_batch_tables", C.c_int, [_vp, C.c_int, C.c_int, C.c_int, _dp, C.c_int64, _ip, _ip, C.c_int, _dp, _dp, _ip, _dp, _vp, _ip, _dp,
                                            _ip, _ip, _ip, C.POINTER(C.c_int)]),
    ("tamcmc_hip_get_rgb_adjoint_stats", C.c_int, [_vp, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    ("tamcmc_hip_get_rgb_adjoint_times", C.c_int, [_vp, _dp]),
    ("tamcmc_hip_model_stats_create", C.c_int, [C.POINTER(_vp), _vp, C.c_int, _dp, C.c_int64, _ip, _ip, C.c_int32]),
    ("tamcmc_hip_model_stats_add_params", C.c_int, [_vp, C.c_int64, _dp, C.c_int64, _dp]),
    ("tamcmc_hip_model_stats_add_vars", C.c_int, [_vp, C.c_int64, _dp, C.c_int64, _dp]),
    ("tamcmc_hip_model_stats_get", C.c_int, [_vp, _dp, C.POINTER(C.c_int64), _dp, _dp, _dp, _dp, _dp, _dp]),
    ("tamcmc_hip_model_stats_reset", C.c_int, [_vp]),
    ("tamcmc_hip_model_stats_destroy", None, [_vp]),
]

_lib = None


def lib():
    """Loads libtamcmc_hip.so (never builds it silently, never falls back)."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f"{LIB_PATH} is missing: run `make -C {_HERE}` (or __graft_entry__.build()) first; "
                               "there is no CPU fallback for the product path")
        _lib = C.CDLL(LIB_PATH)
        for name, res, args in ABI + EXTRA_ABI:
            f = getattr(_lib, name)
            f.restype = res
            f.argtypes = args
    return _lib


EXTRA_ABI = []  # filled by sampler.py (include/tamcmc_sampler.h)


class TamcmcError(RuntimeError):
    def __init__(self, code, msg=""):
        super().__init__(f"tamcmc_hip error {code}: {msg}")
        self.code = code


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a, t=_dp):
    return a.ctypes.data_as(t) if a is not None else None


def pinned_empty(shape, dtype=np.float64):
    """A numpy array in page-locked host memory (tamcmc_hip_host_alloc): the record buffers of Sampler.run(out=...) are then filled by
    an asynchronous DMA.  Freed when the array (and every view of it) is garbage-collected."""
    L = lib()
    n = int(np.prod(shape)) * np.dtype(dtype).itemsize
    p = L.tamcmc_hip_host_alloc(max(n, 1))
    if not p:
        raise MemoryError("tamcmc_hip_host_alloc failed")
    buf = (C.c_char * max(n, 1)).from_address(p)
    arr = np.frombuffer(buf, dtype=dtype, count=int(np.prod(shape))).reshape(shape)
    weakref.finalize(buf, L.tamcmc_hip_host_free, p)
    return arr


def build_mode_table(model_id, params, plength, x):
    """Host-side table builder (no GPU needed). Returns (status, mults[structured], noise_abs, nharvey)."""
    L = lib()
    params, plength, x = _f64(params), _i32(plength), _f64(x)
    cap = 4096
    mults = np.zeros(cap, dtype=MULT_DTYPE)
    noise = np.zeros(max(int(plength[8]), 1))
    n, nh, nn = C.c_int(0), C.c_int(0), C.c_int(0)
    st = L.tamcmc_build_mode_table(int(model_id), _p(params), _p(plength, _ip), _p(x), x.size, mults.ctypes.data, cap,
                                   C.byref(n), _p(noise), C.byref(nh), C.byref(nn))
    return st, mults[:min(n.value, cap)].copy(), noise[:max(nn.value, 0)].copy(), nh.value


class HipContext:
    """One context = one GPU + one HIP stream + the resident spectrum (tamcmc_hip_ctx)."""

    def __init__(self, device=0, precision=PRECISION_STRICT, timing=False, bins_per_thread=None, workgroup=None):
        self._L = lib()
        h = _vp()
        st = self._L.tamcmc_hip_create(C.byref(h), int(device))
        if st != OK:
            raise TamcmcError(st, "tamcmc_hip_create failed (no GPU / HIP runtime?) -- there is no CPU fallback")
        self._h = h
        self._samplers = weakref.WeakSet()  # samplers borrow the context: they are destroyed first, whatever order the caller (or the GC) uses
        self._model_stats = weakref.WeakSet()  # ModelStats handles borrow the context too
        self.Nx = 0
        self.set_option(OPT_PRECISION, precision)
        self.set_option(OPT_TIMING, 1 if timing else 0)
        if workgroup:
            self.set_option(OPT_WORKGROUP, workgroup)
        if bins_per_thread:
            self.set_option(OPT_BINS_PER_THREAD, bins_per_thread)

    def close(self):
        if getattr(self, "_h", None):
            for smp in list(getattr(self, "_samplers", ())):
                smp.close()
            for ms in list(getattr(self, "_model_stats", ())):
                ms.close()
            self._L.tamcmc_hip_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, st, tolerate=()):
        if st != OK and st not in tolerate:
            raise TamcmcError(st, self._L.tamcmc_hip_last_error(self._h).decode())
        return st

    def set_option(self, opt, value):
        self._chk(self._L.tamcmc_hip_set_option(self._h, int(opt), int(value)))

    def set_spectrum(self, x, y):
        x, y = _f64(x), _f64(y)
        assert x.shape == y.shape and x.ndim == 1
        self._chk(self._L.tamcmc_hip_set_spectrum(self._h, _p(x), _p(y), x.size))
        self.Nx = x.size

    def loglike_batch(self, mults, offsets, noise, nharvey, nnoise, Tcoefs=None, p=1.0, want_model=False):
        mults = np.ascontiguousarray(mults, dtype=MULT_DTYPE)
        offsets, nharvey, nnoise = _i32(offsets), _i32(nharvey), _i32(nnoise)
        noise = _f64(noise)
        B = nharvey.size
        noise = noise.reshape(B, -1)
        T = _f64(Tcoefs) if Tcoefs is not None else None
        logL = np.zeros(B)
        model = np.zeros((B, self.Nx)) if want_model else None
        st = self._L.tamcmc_hip_loglike_batch(self._h, B, mults.ctypes.data, _p(offsets, _ip), _p(noise), noise.shape[1],
                                             _p(nharvey, _ip), _p(nnoise, _ip), _p(T), float(p), _p(logL), _p(model))
        self._chk(st)
        return logL, model

    def loglike_params_batch(self, model_id, params, plength, Tcoefs=None, p=1.0, want_model=False):
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        B, Np = params.shape
        plength = _i32(plength)
        T = _f64(Tcoefs) if Tcoefs is not None else None
        logL = np.zeros(B)
        model = np.zeros((B, self.Nx)) if want_model else None
        status = np.zeros(B, dtype=np.int32)
        st = self._L.tamcmc_hip_loglike_params_batch(self._h, int(model_id), B, _p(params), Np, _p(plength, _ip), _p(T),
                                                    float(p), _p(logL), _p(model), _p(status, _ip))
        # a per-vector table failure comes back as the call's code AND in status[b] (that vector's logL is NaN): not an exception
        self._chk(st, tolerate=(ERR_EMPTY_WINDOW, ERR_NAN_WINDOW) + ((int(st),) if (status != OK).any() else ()))
        return logL, model, status

    def fd_gradient(self, model_id, params, plength, index_to_relax, hstep, Tcoefs=None, p=1.0):
        """(logL0 [C], grad [C x Nvars]) of the tempered log-likelihood by forward differences, one device-built batch.  Every Lorentzian
        model id with a device table builder, the red giants (25, 27: tables through the device pre-step) and the envelope fits (0, 1)."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        plength, idx, h = _i32(plength), _i32(index_to_relax), _f64(hstep)
        T = _f64(Tcoefs) if Tcoefs is not None else None
        l0 = np.zeros(Cn)
        g = np.zeros((Cn, idx.size))
        st = self._L.tamcmc_hip_fd_gradient(self._h, int(model_id), Cn, _p(params), Np, _p(plength, _ip), _p(idx, _ip),
                                           idx.size, _p(h), _p(T), float(p), _p(l0), _p(g))
        self._chk(st, tolerate=(ERR_EMPTY_WINDOW, ERR_NAN_WINDOW))
        return l0, g

    def fd_gradient_posterior(self, star, params, hstep, Tcoefs=None, p=1.0):
        """Gradient of the tempered log-posterior of `star`'s model at each row of params (device-built FD batch); the prior class must
        be the model's own (red giants, ids 25 / 27: class 4).  The prior's share is left in self.last_grad_prior."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        plength, idx, h = _i32(star.plength), _i32(star.index_to_relax), _f64(hstep)
        pri, sw, ex = _f64(star.priors), _i32(star.priors_switch), _f64(star.extra_priors)
        T = _f64(Tcoefs) if Tcoefs is not None else None
        l0, pr0, g, gp = np.zeros(Cn), np.zeros(Cn), np.zeros((Cn, idx.size)), np.zeros((Cn, idx.size))
        st = self._L.tamcmc_hip_fd_gradient_posterior(self._h, int(star.model_id), int(star.prior_class), Cn, _p(params), Np,
                                                     _p(plength, _ip), _p(idx, _ip), idx.size, _p(h), _p(T), float(p), _p(pri),
                                                     _p(sw, _ip), _p(ex), _p(l0), _p(pr0), _p(g), _p(gp))
        self._chk(st, tolerate=(ERR_EMPTY_WINDOW, ERR_NAN_WINDOW))
        self.last_grad_prior = gp
        return l0, pr0, g

    def adjoint_table(self, model_id, params, plength, Tcoefs=None, p=1.0):
        """Table-space adjoint of the un-tempered sum S at each row of params (tamcmc_hip_adjoint_table): (G [C x rows x 17], Gn [C x nnoise]),
        fields of G in the order nu[7], hv[7], gamma, asym, fc.  Red giants (ids 25 / 27, with OPT_RGB_ADJOINT): rows = the rows reserved
        per table, zeros beyond a table's own."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        plength = _i32(plength)
        T = _f64(Tcoefs) if Tcoefs is not None else None
        n = C.c_int(0)
        self._chk(self._L.tamcmc_hip_adjoint_table(self._h, int(model_id), 0, _p(params), Np, _p(plength, _ip), _p(T), float(p), None, None,
                                                   C.byref(n)))
        G = np.zeros((Cn, n.value, 17))
        Gn = np.zeros((Cn, max(int(plength[8]), 1)))
        self._chk(self._L.tamcmc_hip_adjoint_table(self._h, int(model_id), Cn, _p(params), Np, _p(plength, _ip), _p(T), float(p), _p(G), _p(Gn),
                                                   C.byref(n)))
        return G, Gn

    def envelope_gradient_sums(self, model_id, params):
        """Row-space sums of the envelope fits' analytic gradient, before the chain rule (tamcmc_hip_envelope_gradient_sums; ids 0 / 1):
        (S [C], sums [C x 13] = dS/d(row quantity), ksi [C x 9] -- the xi sums I_k, I_k^b, I_k^c of id 0, zeros for id 1)."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        S, sums, ksi = np.zeros(Cn), np.zeros((Cn, ENVELOPE_GRAD_N)), np.zeros((Cn, ENVELOPE_KSI_N))
        self._chk(self._L.tamcmc_hip_envelope_gradient_sums(self._h, int(model_id), Cn, _p(params), Np, _p(S), _p(sums), _p(ksi)))
        return S, sums, ksi

    def rgb_batch_tables(self, model_id, params, plength, index_to_relax, hstep):
        """The tables of a red-giant gradient batch as its own builder leaves them (tamcmc_hip_rgb_batch_tables), in batch order: slot
        c (Nvars + 1) is chain c's vector, slot c (Nvars + 1) + 1 + k the same with hstep[k] added to index_to_relax[k].  Returns
        (tables, noise, nharvey, status): tables[slot] = that slot's rows (MULT_DTYPE), noise[slot] = its |noise| row (nnoise values)."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        plength, idx, h = _i32(plength), _i32(index_to_relax), _f64(hstep)
        assert h.size == idx.size
        per = C.c_int(0)
        args = (int(model_id), _p(params), Np, _p(plength, _ip), _p(idx, _ip), idx.size, _p(h))
        self._chk(self._L.tamcmc_hip_rgb_batch_tables(self._h, args[0], 0, *args[1:], None, None, None, None, None, None, C.byref(per)))
        B, stride = Cn * (idx.size + 1), max(int(plength[8]), 1)
        rows = np.zeros((B, per.value), dtype=MULT_DTYPE)
        n, nh, nn, status = (np.zeros(B, dtype=np.int32) for _ in range(4))
        noise = np.zeros((B, stride))
        st = self._L.tamcmc_hip_rgb_batch_tables(self._h, args[0], Cn, *args[1:], rows.ctypes.data, _p(n, _ip), _p(noise), _p(nh, _ip),
                                                 _p(nn, _ip), _p(status, _ip), C.byref(per))
        # a per-vector table failure comes back as the call's code AND in status[slot] (that slot's table is empty): not an exception
        self._chk(st, tolerate=((int(st),) if (status != OK).any() else ()))
        return [rows[s, :n[s]].copy() for s in range(B)], [noise[s, :max(nn[s], 0)].copy() for s in range(B)], nh, status

    def fd_batch_tables(self, model_id, params, plength, index_to_relax, hstep, star=None):
        """The tables of a main-sequence gradient batch as its table kernel leaves them (tamcmc_hip_fd_batch_tables), in batch order like
        rgb_batch_tables.  star: evaluate its log-prior in front of the unpack (the fd_gradient_posterior path); None: no prior class.
        Returns (tables, noise, nharvey, nnoise, status)."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        plength, idx, h = _i32(plength), _i32(index_to_relax), _f64(hstep)
        assert h.size == idx.size
        pc, pri, sw, ex = 0, None, None, None
        if star is not None:
            pc, pri, sw, ex = int(star.prior_class), _f64(star.priors), _i32(star.priors_switch), _f64(star.extra_priors)
        per = C.c_int(0)
        head = (int(model_id), pc)
        args = (_p(params), Np, _p(plength, _ip), _p(idx, _ip), idx.size, _p(h), _p(pri), _p(sw, _ip), _p(ex))
        self._chk(self._L.tamcmc_hip_fd_batch_tables(self._h, *head, 0, *args, None, None, None, None, None, None, C.byref(per)))
        B, stride = Cn * (idx.size + 1), max(int(plength[8]), 1)
        rows = np.zeros((B, per.value), dtype=MULT_DTYPE)
        n, nh, nn, status = (np.zeros(B, dtype=np.int32) for _ in range(4))
        noise = np.zeros((B, stride))
        st = self._L.tamcmc_hip_fd_batch_tables(self._h, *head, Cn, *args, rows.ctypes.data, _p(n, _ip), _p(noise), _p(nh, _ip), _p(nn, _ip),
                                                _p(status, _ip), C.byref(per))
        # a per-vector table failure comes back as the call's code AND in status[slot] (that slot holds the placeholder): not an exception
        self._chk(st, tolerate=((int(st),) if (status != OK).any() else ()))
        return [rows[s, :n[s]].copy() for s in range(B)], noise, nh, nn, status

    def rgb_adjoint_stats(self):
        """(linearised slots, fallback slots) of the hybrid red-giant adjoint batches since the last reset (timing on)."""
        a, b = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.tamcmc_hip_get_rgb_adjoint_stats(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def rgb_adjoint_times(self):
        """HIP-event split of the last hybrid batch of a host entry, ms (timing on): table build, base launch, row pass, noise pass +
        folds, fallback delta launches, contraction."""
        t = np.zeros(6)
        self._chk(self._L.tamcmc_hip_get_rgb_adjoint_times(self._h, _p(t)))
        return tuple(t)

    def fisher(self, model_id, params, plength, index_to_relax, hstep, Tcoefs=None, p=1.0):
        """Expected (Fisher) information F [C x Nvars x Nvars] of the likelihood at each row of params (tamcmc_hip_fisher): central
        differences with frozen windows, F = (p / T) U U^T (red giants, with OPT_RGB_FISHER: per variable the central, the one-sided or the
        unfrozen form, include/tamcmc_hip.h).  A table that fails at a perturbed point leaves NaN in that row and column;
        the status of the call is left in self.last_fisher_status."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        Cn, Np = params.shape
        plength, idx, h = _i32(plength), _i32(index_to_relax), _f64(hstep)
        assert h.size == idx.size
        T = _f64(Tcoefs) if Tcoefs is not None else None
        F = np.zeros((Cn, idx.size, idx.size))
        st = self._L.tamcmc_hip_fisher(self._h, int(model_id), Cn, _p(params), Np, _p(plength, _ip), _p(idx, _ip), idx.size, _p(h), _p(T),
                                      float(p), _p(F))
        self.last_fisher_status = self._chk(st, tolerate=(ERR_EMPTY_WINDOW, ERR_NAN_WINDOW))
        return F

    def fisher_times(self):
        """(table build, row launches, Gram + fold) of the last fisher() call in ms (HIP events; the context's timing option on)."""
        a, b, g = C.c_double(0), C.c_double(0), C.c_double(0)
        self._chk(self._L.tamcmc_hip_get_fisher_times(self._h, C.byref(a), C.byref(b), C.byref(g)))
        return a.value, b.value, g.value

    def rgb_fisher_stats(self):
        """(central, one-sided, unfrozen) (chain, variable) pairs of the last fisher() call on a red giant (OPT_RGB_FISHER; timing on)."""
        a, b, u = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._L.tamcmc_hip_get_rgb_fisher_stats(self._h, C.byref(a), C.byref(b), C.byref(u)))
        return a.value, b.value, u.value

    def weighted_gram(self, A, w=None):
        """G [N x N] = sum_k w_k A_jk A_lk through the Gram and fold kernels of fisher() (tamcmc_hip_weighted_gram; w None: ones)."""
        A = _f64(A)
        assert A.ndim == 2
        w = _f64(w) if w is not None else None
        assert w is None or w.shape == (A.shape[1],)
        G = np.zeros((A.shape[0], A.shape[0]))
        self._chk(self._L.tamcmc_hip_weighted_gram(self._h, A.shape[0], A.shape[1], _p(A), _p(w), _p(G)))
        return G

    def rgb_mixed_modes(self, model_id, params, plength, max_modes=1024):
        """l=1 mixed modes of one red-giant vector from the device pre-step: (nu_m, zeta, H1/H0) -- what ARMM's do_solve prints."""
        params, plength = _f64(params), _i32(plength)
        nu, z, h = np.zeros(max_modes), np.zeros(max_modes), np.zeros(max_modes)
        n = C.c_int(0)
        self._chk(self._L.tamcmc_hip_rgb_mixed_modes(self._h, int(model_id), _p(params), params.size, _p(plength, _ip), max_modes,
                                                     _p(nu), _p(z), _p(h), C.byref(n)))
        k = min(n.value, max_modes)
        return nu[:k].copy(), z[:k].copy(), h[:k].copy()

    def kernel_stats(self):
        ms, n, e = C.c_double(0), C.c_int64(0), C.c_int64(0)
        self._chk(self._L.tamcmc_hip_get_kernel_stats(self._h, C.byref(ms), C.byref(n), C.byref(e)))
        return ms.value, n.value, e.value

    def fd_stats(self):
        """(bins inside the affected ranges, delta evaluations) of the windowed finite-difference launches since the last reset."""
        b, e = C.c_int64(0), C.c_int64(0)
        self._chk(self._L.tamcmc_hip_get_fd_stats(self._h, C.byref(b), C.byref(e)))
        return b.value, e.value

    def fd_full_tables(self):
        """Delta evaluations since the last reset that were evaluated as whole perturbed tables (timing on)."""
        n = C.c_int64(0)
        self._chk(self._L.tamcmc_hip_get_fd_full_tables(self._h, C.byref(n)))
        return n.value

    def reset_kernel_stats(self):
        self._chk(self._L.tamcmc_hip_reset_kernel_stats(self._h))

    def model_stats(self, star_or_model_id, inputs=None, plength=None, relax=None, chunk=0):
        """Posterior model spectrum of this context's spectrum (tamcmc_hip_model_stats_*): a ModelStats accumulator for a synth.Star /
        inputs.Star-like object (model_id, params, plength, relax) or for a model id with inputs, plength and, for add_vars, relax."""
        if hasattr(star_or_model_id, "model_id"):
            s = star_or_model_id
            return ModelStats(self, s.model_id, s.params if inputs is None else inputs, s.plength, s.relax, chunk)
        return ModelStats(self, star_or_model_id, inputs, plength, relax, chunk)


class ModelStats:
    """Per-bin mean, variance, envelope, mean y/M and mean background of the model over a stream of parameter vectors, accumulated on the
    device (include/tamcmc_hip.h, "posterior model spectrum").  Borrows its HipContext: close it before the context."""

    def __init__(self, ctx, model_id, inputs, plength, relax=None, chunk=0):
        self._ctx, self._L = ctx, ctx._L
        inputs, plength = _f64(inputs), _i32(plength)
        relax = _i32(relax) if relax is not None else None
        assert relax is None or relax.size == inputs.size
        self.Nparams = inputs.size
        self.Nvars = int((relax == 1).sum()) if relax is not None else 0
        h = _vp()
        st = self._L.tamcmc_hip_model_stats_create(C.byref(h), ctx._h, int(model_id), _p(inputs), inputs.size, _p(relax, _ip), _p(plength, _ip),
                                                  int(chunk))
        if st != OK:
            raise TamcmcError(st, "tamcmc_hip_model_stats_create")
        self._h = h
        self.Nx = ctx.Nx
        ctx._model_stats.add(self)

    def _chk(self, st):
        if st != OK:
            raise TamcmcError(st, self._L.tamcmc_hip_last_error(self._ctx._h).decode())

    @staticmethod
    def _weights(weights, n):
        if weights is None:
            return None
        w = _f64(weights)
        assert w.shape == (n,)
        return w

    def add_params(self, params, weights=None):
        """params [n x Nparams] (or one vector); weights [n] or None (all 1)."""
        params = _f64(params)
        if params.ndim == 1:
            params = params[None, :]
        assert params.ndim == 2 and params.shape[1] == self.Nparams
        w = self._weights(weights, params.shape[0])
        self._chk(self._L.tamcmc_hip_model_stats_add_params(self._h, params.shape[0], _p(params), self.Nparams, _p(w)))

    def add_vars(self, vars_, chain=0, weights=None):
        """vars_ [n x Nvars] rows of the free variables, or a Sampler.run record [n x Nchains x Nvars] of which `chain` is taken in place."""
        v = _f64(vars_)
        if v.ndim == 1:
            v = v[None, :]
        if v.ndim == 3:
            n, nch, nv = v.shape
            assert 0 <= chain < nch
            stride, first = nch * nv, v.reshape(-1)[chain * nv:]
        else:
            (n, nv), stride, first = v.shape, v.shape[1], v
        assert nv == self.Nvars
        w = self._weights(weights, n)
        self._chk(self._L.tamcmc_hip_model_stats_add_vars(self._h, n, _p(first) if n else None, stride, _p(w)))

    def result(self):
        """dict: mean, var, min, max, ratio, background ([Nx] each), W, and counts = (accepted, failed tables, zero weights)."""
        out = {k: np.zeros(self.Nx) for k in ("mean", "var", "min", "max", "ratio", "background")}
        W, counts = C.c_double(0), (C.c_int64 * 3)()
        self._chk(self._L.tamcmc_hip_model_stats_get(self._h, C.byref(W), counts, *(_p(out[k]) for k in ("mean", "var", "min", "max", "ratio",
                                                                                                       "background"))))
        out["W"] = W.value
        out["counts"] = tuple(int(c) for c in counts)
        return out

    def reset(self):
        self._chk(self._L.tamcmc_hip_model_stats_reset(self._h))

    def close(self):
        if getattr(self, "_h", None):
            self._L.tamcmc_hip_model_stats_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


from . import sampler  # noqa: E402,F401  (registers the tamcmc_sampler_* symbols in EXTRA_ABI)
from . import inputs  # noqa: E402,F401  (include/tamcmc_io.h)
from .sampler import Sampler  # noqa: E402,F401
