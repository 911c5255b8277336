"""Target distributions of the geodesic slice sampler, API-compatible with
geosss/distributions.py for the families the hot path covers:

    VonMisesFisher(mu)                      distributions.py:117-160
    MixtureModel(components, weights=None)  distributions.py:209-227 (components: vMF, Bingham, BinghamFisher,
                                            Uniform, CurvedVonMisesFisher, MixtureModel)
    Bingham(A), random_bingham(...)         distributions.py:36-103, 230-258
    CurvedVonMisesFisher(curve, kappa)      distributions.py:261-278
    SlerpCurve(knots), brownian_curve(...)  spherical_curve.py:74-129

The objects are parameter carriers: they keep the same attributes as the reference
(`.mu`, `.pdfs`, `.weights`, `.A`, `.curve.knots`, `.kappa`, `.d`) and hand a packed
parameter block to the HIP library.  `log_prob` accepts a point (d,) or rows (n, d), as in
the reference, and is evaluated ON THE GPU through the C ABI (`gsss_logprob`); there is no
host implementation to fall back to.  `pdf.log_prob.num_calls` / `.reset_counters()` keep
the reference's call-counter protocol (utils.py:137-185); the samplers add the number of
log-density evaluations their kernels performed.
"""
import ctypes as C

import numpy as np
import torch
from scipy.special import i0, ive, iv, logsumexp

from . import _lib
from .sphere import _device_index, current_stream_ptr

__all__ = ["Distribution", "VonMisesFisher", "MixtureModel", "Bingham", "BinghamFisher", "CurvedVonMisesFisher", "SlerpCurve",
           "TargetBatch", "random_bingham", "brownian_curve", "counted"]


def counted(fn):
    """Call counter with the reference's protocol: `obj.method.num_calls`, `obj.method.reset_counters()`
    (the attributes live on the underlying function, so they are shared by all instances of the
    class, exactly like geosss.utils.count_calls)."""

    def method(self, *args, **kwargs):
        method.num_calls += 1
        return fn(self, *args, **kwargs)

    def reset_counters():
        method.num_calls = 0

    method.num_calls = 0
    method.reset_counters = reset_counters
    method.__name__ = fn.__name__
    method.__doc__ = fn.__doc__
    return method


def _as_f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def log_bessel_i0(kappa):
    """log(i0(kappa)).  The reference evaluates np.log(i0(kappa)) (distributions.py:157), which
    overflows to +inf for kappa >~ 713.99 and then never terminates (mcmc.py:394); below that
    threshold we return the very same expression, above it the overflow-free equivalent
    log(ive(0, kappa)) + kappa."""
    kappa = np.asarray(kappa, dtype=np.float64)
    with np.errstate(over="ignore"):
        direct = np.log(i0(kappa))
    safe = np.log(ive(0, kappa)) + kappa
    return np.where(np.isfinite(direct), direct, safe)


class _DeviceTarget:
    """Owns one gsss_target handle (device parameter block)."""

    def __init__(self, desc_arrays, kind, d, k, kappa, device, extra=None):
        _lib.require_device()
        self.lib = _lib.load()
        self.device = device
        self._keep = (desc_arrays, extra)  # keep the host arrays alive during create
        if kind == _lib.MIXTURE:  # extra: the components' packs and their log weights (MixtureModel._pack)
            comps = extra["components"]
            descs = (_lib.TargetDesc * len(comps))()
            for i, (ckind, cd, ck, ckappa, arrays) in enumerate(comps):
                descs[i] = _lib.TargetDesc(ckind, cd, ck, 0,
                                           *[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays],
                                           float(ckappa))
            logw = extra["log_weights"]
            h = C.c_void_p()
            _lib.check(self.lib.gsss_target_create_mixture(descs, len(comps), logw.ctypes.data_as(C.c_void_p), device,
                                                           C.byref(h)))
            self.handle = h
            return
        if extra is not None and "batch" in extra:  # extra: the members' packs and the chains per target (TargetBatch._pack)
            members = extra["batch"]
            descs = (_lib.TargetDesc * len(members))()
            for i, (mkind, md, mk, mkappa, arrays) in enumerate(members):
                descs[i] = _lib.TargetDesc(mkind, md, mk, 0,
                                           *[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in arrays],
                                           float(mkappa))
            h = C.c_void_p()
            _lib.check(self.lib.gsss_target_create_batch(descs, len(members), int(extra["chains_per_target"]), device, C.byref(h)))
            self.handle = h
            return
        if kind == _lib.USER:  # extra: the compiled module's table (usertarget.DeviceDistribution._pack)
            (p,) = desc_arrays
            h = C.c_void_p()
            _lib.check(self.lib.gsss_target_create_user(C.c_void_p(extra["table"]), d, p.ctypes.data_as(C.c_void_p) if p.size else None,
                                                        p.size, device, C.byref(h)))
            self.handle = h
            return
        desc = _lib.TargetDesc(kind, d, k, 0,
                               *[a.ctypes.data_as(C.c_void_p) if a is not None else None for a in desc_arrays],
                               float(kappa))
        for name, value in (extra or {}).items():  # registration targets: the further fields of gsss_target_desc
            setattr(desc, name, value.ctypes.data_as(C.c_void_p) if isinstance(value, np.ndarray) else value)
        h = C.c_void_p()
        _lib.check(self.lib.gsss_target_create(C.byref(desc), device, C.byref(h)))
        self.handle = h

    def __del__(self):
        try:
            if getattr(self, "handle", None):
                self.lib.gsss_target_destroy(self.handle)
                self.handle = None
        except Exception:
            pass


class Distribution:
    """Base class: packing + device evaluation shared by all targets."""

    def _pack(self):
        """-> (kind, d, k, kappa, (mu, logc, A, knots))"""
        raise TypeError(f"{type(self).__name__} has no device parameter block: the samplers run inside HIP kernels and cannot call a "
                        "Python log_prob; built-in targets are VonMisesFisher, Bingham, BinghamFisher, CurvedVonMisesFisher, "
                        "Uniform, MixtureModel (of any of these), AngularCentralGaussian, CoherentPointDrift and GaussianMixtureModel")

    def _device_target(self, device=None):
        dev = _device_index(device)
        packed = self._pack()
        kind, d, k, kappa, arrays = packed[:5]
        extra = packed[5] if len(packed) > 5 else None
        key = self._device_key(packed)
        cache = self.__dict__.setdefault("_targets", {})
        hit = cache.get(dev)
        if hit is None or hit[0] != key:
            cache[dev] = (key, _DeviceTarget(arrays, kind, d, k, kappa, dev, extra))
        return cache[dev][1]

    @staticmethod
    def _device_key(packed):
        # the parameter attributes are public and mutable, as in the reference: key the device copy on
        # their current bytes so that an edited target is re-uploaded instead of silently reused
        kind, d, k, kappa, arrays = packed[:5]
        extra = packed[5] if len(packed) > 5 else None
        key = (kind, d, k, kappa) + tuple(a.tobytes() if a is not None else None for a in arrays)
        if extra and kind == _lib.MIXTURE:  # every component's parameter bytes: editing pdfs[1].A re-uploads
            key += tuple((c[:4],) + tuple(a.tobytes() if a is not None else None for a in c[4]) for c in extra["components"])
            key += (extra["log_weights"].tobytes(),)
        elif extra:
            key += tuple(v.tobytes() if isinstance(v, np.ndarray) else v for v in extra.values())
        return key

    def _invalidate(self):
        self.__dict__.pop("_targets", None)

    def _log_prob_device(self, x):
        """x: numpy (d,), (n, d) or a CUDA float64 tensor (n, d) -> same kind of container."""
        if isinstance(x, torch.Tensor):
            if not x.is_cuda:
                raise ValueError("torch input to log_prob must live on the GPU")
            tgt = self._device_target(x.device)
            xt = x.to(torch.float64).contiguous()
            single = xt.ndim == 1
            xt2 = xt[None] if single else xt
            if xt2.ndim != 2 or xt2.shape[1] != self.d:
                raise ValueError(f"expected (..., {self.d}) input")
            out = torch.empty(xt2.shape[0], dtype=torch.float64, device=xt.device)
            dev = _device_index(xt.device)
            _lib.check(tgt.lib.gsss_logprob(tgt.handle, xt2.data_ptr(), xt2.shape[0], out.data_ptr(),
                                            current_stream_ptr(dev)))
            return out[0] if single else out
        x = np.asarray(x, dtype=np.float64)
        if x.ndim not in (1, 2) or x.shape[-1] != self.d:
            raise ValueError(f"expected (d,) or (n, d) input with d={self.d}")  # distributions.py:84
        _lib.require_device()
        dev = _device_index(None)
        xt = torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x))).to(f"cuda:{dev}")
        out = self._log_prob_device(xt).cpu().numpy()
        return float(out[0]) if x.ndim == 1 else out

    def _gradient_device(self, x):
        """Distribution.gradient through gsss_gradient (the functions the spherical HMC kernel evaluates): numpy (d,) or (n, d),
        or a CUDA float64 tensor (n, d) -> the same kind of container."""
        if isinstance(x, torch.Tensor):
            if not x.is_cuda:
                raise ValueError("torch input to gradient must live on the GPU")
            tgt = self._device_target(x.device)
            xt = x.to(torch.float64).contiguous()
            single = xt.ndim == 1
            xt2 = xt[None] if single else xt
            if xt2.ndim != 2 or xt2.shape[1] != self.d:
                raise ValueError(f"expected (..., {self.d}) input")
            out = torch.empty_like(xt2)
            dev = _device_index(xt.device)
            _lib.check(tgt.lib.gsss_gradient(tgt.handle, xt2.data_ptr(), xt2.shape[0], out.data_ptr(), current_stream_ptr(dev)))
            return out[0] if single else out
        x = np.asarray(x, dtype=np.float64)
        if x.ndim not in (1, 2) or x.shape[-1] != self.d:
            raise ValueError(f"expected (d,) or (n, d) input with d={self.d}")
        _lib.require_device()
        dev = _device_index(None)
        out = self._gradient_device(torch.from_numpy(np.ascontiguousarray(np.atleast_2d(x))).to(f"cuda:{dev}")).cpu().numpy()
        return out[0] if x.ndim == 1 else out

    def log_prob(self, x):
        raise NotImplementedError

    def gradient(self, x):
        """The gradient of log_prob in the ambient space, as the reference's classes define it; evaluated on the device."""
        return self._gradient_device(x)


class VonMisesFisher(Distribution):
    """vMF(x) ~ exp(mu.x);  log_prob = x.mu - log(2 pi) - log(i0(|mu|))  (distributions.py:156-157).
    `mu` is stored unnormalised, kappa = |mu| (distributions.py:126-136)."""

    def __init__(self, mu):
        self.mu = np.array(mu, dtype=np.float64)

    @property
    def d(self):
        return self.mu.size

    @property
    def kappa(self):
        return float(np.linalg.norm(self.mu))

    @property
    def mode(self):
        return self.mu / (np.linalg.norm(self.mu) + 1e-100)

    @property
    def max_log_prob(self):
        return self.kappa

    def _log_const(self):
        return -np.log(2 * np.pi) - float(log_bessel_i0(self.kappa))

    def _pack(self):
        mu = _as_f64(self.mu[None])
        logc = _as_f64([self._log_const()])
        return _lib.VMF_MIXTURE, self.d, 1, 0.0, (mu, logc, None, None)

    @counted
    def log_prob(self, x):
        return self._log_prob_device(x)

    @counted
    def gradient(self, x):
        return self.mu                                  # distributions.py:159-160 (whatever the shape of x)


class _HostDensity(Distribution):
    """Densities the reference defines beside its sampler targets (plot overlays, envelopes): evaluated on the host with
    numpy, as the reference does; they have no device parameter block and are refused as targets of the HIP samplers."""

    def _pack(self):
        raise TypeError(f"{type(self).__name__} is a host-side density (plotting / envelope); the HIP samplers run on "
                        "VonMisesFisher, Bingham, BinghamFisher, CurvedVonMisesFisher, Uniform, MixtureModel (of any of these), "
                        "AngularCentralGaussian and the registration targets")


class MarginalVonMisesFisher(_HostDensity, VonMisesFisher):
    """The density on [-1, 1] of coordinate `dim_idx` of a vMF(mu) variate (distributions.py:164-186): what the
    reference's diagnostics overlay on the histograms of the chains' coordinates."""

    def __init__(self, dim_idx, mu):
        VonMisesFisher.__init__(self, mu)
        self.dim_idx = dim_idx

    def prob(self, x):
        x = np.asarray(x, dtype=np.float64)
        d, kappa = self.d, self.kappa
        m = self.mu[self.dim_idx] / kappa                        # the mean direction's own coordinate
        rest = (1.0 - m * m) * (1.0 - x * x)
        return (np.sqrt(kappa / (2.0 * np.pi)) / iv(0.5 * d - 1.0, kappa) * ((1.0 - x * x) / (1.0 - m * m)) ** (0.25 * (d - 3))
                * np.exp(kappa * m * x) * iv(0.5 * (d - 3), kappa * np.sqrt(rest)))

    @counted
    def log_prob(self, x):
        return np.log(np.clip(self.prob(x), 1e-308, None))


class MultivariateNormal(_HostDensity):
    """-(x - mu)^T C^-1 (x - mu) / 2 (distributions.py:189-197)."""

    def __init__(self, mu, C):
        self.mu = np.asarray(mu, dtype=np.float64)
        self.C = np.asarray(C, dtype=np.float64)
        self.invC = np.linalg.inv(self.C)

    @property
    def d(self):
        return len(self.C)

    def _quad(self, x):
        r = np.asarray(x, dtype=np.float64) - self.mu
        return np.sum(r * (r @ self.invC), axis=-1)

    @counted
    def log_prob(self, x):
        return -0.5 * self._quad(x)


class ACG(MultivariateNormal):
    """Angular central Gaussian: -(d / 2) log(x^T C^-1 x) (distributions.py:200-207); the envelope of rand.sample_bingham."""

    def __init__(self, C):
        super().__init__(np.zeros(len(C)), C)

    @counted
    def log_prob(self, x):
        return -0.5 * self.d * np.log(self._quad(x))


class AngularCentralGaussian(Distribution):
    """Angular central Gaussian as a sampler target: log_prob = -(d / 2) log(x^T Lambda x), unnormalised, with the precision
    matrix Lambda = C^-1 symmetric positive definite (distributions.py:199-206 with invC = Lambda).  Runs on kernels of its own
    (GSSS_ACG): both slice samplers in exact and, at d = 3 .. 10, fast mode, and the four Metropolis-Hastings / HMC classes;
    log_prob and gradient = -d Lambda x / (x^T Lambda x) are evaluated on the device.  `ACG` stays the host-side overlay;
    `.host()` gives the equivalent one.  Not a MixtureModel component or TargetBatch member."""

    def __init__(self, precision):
        L = np.array(precision, dtype=np.float64)
        if L.ndim != 2 or L.shape[0] != L.shape[1] or L.shape[0] < 2 or not np.all(np.isfinite(L)):
            raise ValueError("precision must be a finite square matrix (d >= 2)")
        if not np.max(np.abs(L - L.T)) <= 1e-10 * np.max(np.abs(L)):  # (rounding of an inverse or of Q diag Q^T passes)
            raise ValueError("precision must be symmetric")
        L = 0.5 * (L + L.T)  # symmetric to the last bit, which the library asks for
        try:
            np.linalg.cholesky(L)
        except np.linalg.LinAlgError:
            raise ValueError("precision must be positive definite") from None
        self.precision = L

    @classmethod
    def from_covariance(cls, C):
        """The target with Lambda = C^-1."""
        C = np.array(C, dtype=np.float64)
        if C.ndim != 2 or C.shape[0] != C.shape[1]:
            raise ValueError("C must be a square matrix")
        return cls(np.linalg.inv(C))

    @property
    def d(self):
        return len(self.precision)

    @property
    def mode(self):
        """An axis of largest density (the density is antipodally symmetric): the eigenvector of Lambda's smallest eigenvalue."""
        return np.linalg.eigh(self.precision)[1][:, 0]

    @property
    def max_log_prob(self):
        return -0.5 * self.d * float(np.log(np.linalg.eigvalsh(self.precision)[0]))

    def host(self):
        """The equivalent host-side `ACG` (covariance Lambda^-1)."""
        return ACG(np.linalg.inv(self.precision))

    def _pack(self):
        return _lib.ACG, self.d, 0, 0.0, (None, None, _as_f64(self.precision), None)

    @counted
    def log_prob(self, x):
        return self._log_prob_device(x)

    @counted
    def gradient(self, x):
        """-d Lambda x / (x^T Lambda x), on the device."""
        return self._gradient_device(x)


class MixtureModel(Distribution):
    """log_prob = logsumexp_k(log_prob_k(x) + log w_k), weights normalised to one (distributions.py:211-221);
    gradient = the softmax-weighted sum of the components' gradients (:223-227).

    Components: VonMisesFisher, Bingham, BinghamFisher, Uniform, CurvedVonMisesFisher and MixtureModel, of one dimension.  A
    nested mixture is flattened (its weights multiply the parent's, its components become terms); a dimensionless Uniform()
    takes the dimension of its siblings, the reference's way of writing an outlier background.  A mixture of vMF terms only
    runs on the vMF-mixture kernels as before; any other runs on the GSSS_MIXTURE kernels.  log_prob and gradient are
    evaluated on the device for a point (d,), rows (n, d) or a CUDA tensor -- rows also with a Uniform component, which the
    reference's batched call does not take.  `log_prob.num_calls` counts the mixture's evaluations as for every target; the
    component objects' own counters do not advance."""

    def __init__(self, components, weights=None):
        self.pdfs = list(components)
        if not self.pdfs:
            raise TypeError("a mixture needs at least one component")
        # a mixture of coordinate marginals (the reference's histogram overlay, scripts/vMF_diagnostics.py:106-108) is a
        # density on [-1, 1]: host arithmetic, never a sampler target
        self._marginal = all(isinstance(p, MarginalVonMisesFisher) for p in self.pdfs)
        if not self._marginal and any(isinstance(p, MarginalVonMisesFisher) for p in self.pdfs):
            raise TypeError("cannot mix coordinate marginals with densities on the sphere")
        if not self._marginal:
            for p in self.pdfs:
                if getattr(p, "_device_source", False):
                    raise TypeError("a DeviceDistribution is not a mixture component on the device: write the mixture in its "
                                    "source instead")
                if isinstance(p, _HostDensity) or not isinstance(p, (VonMisesFisher, Bingham, CurvedVonMisesFisher, MixtureModel)):
                    raise TypeError(f"{type(p).__name__} is not a mixture component on the device: components are VonMisesFisher, "
                                    "Bingham, BinghamFisher, Uniform, CurvedVonMisesFisher and MixtureModel")
                if isinstance(p, MixtureModel) and p._marginal:
                    raise TypeError("cannot mix coordinate marginals with densities on the sphere")
        if len({p.d for p in self.pdfs if p.d is not None}) > 1:
            raise ValueError("all components must share the dimension")
        w = np.ones(len(self.pdfs)) if weights is None else np.array(weights, dtype=np.float64)
        if w.shape != (len(self.pdfs),):
            raise ValueError("one weight per component")
        self.weights = w / w.sum()

    @property
    def d(self):
        for p in self.pdfs:
            if p.d is not None:
                return p.d
        return None

    def _terms(self, d=None):
        """The flattened mixture: [(component, weight)], nested mixtures expanded, Uniform() given the dimension d."""
        d = self.d if d is None else d
        out = []
        for p, w in zip(self.pdfs, self.weights):
            if isinstance(p, MixtureModel):
                out += [(q, w * v) for q, v in p._terms(d)]
            elif isinstance(p, Uniform) and p.d is None and d is not None:
                out.append((Uniform(d), w))
            else:
                out.append((p, w))
        return out

    def _modes(self):
        """Mode directions of the terms that have one (the running statistics' mode occupancy): a vMF term's mu, a Bingham
        term's .mode; Uniform and curve terms have none."""
        return [p.mu if isinstance(p, VonMisesFisher) else p.mode for p, _ in self._terms()
                if isinstance(p, VonMisesFisher) or (isinstance(p, Bingham) and not isinstance(p, Uniform))]

    def _pack(self):
        if self._marginal:
            return _HostDensity._pack(self)
        if self.d is None:
            raise TypeError("a mixture of Uniform() components has no dimension: give one as Uniform(d)")
        terms = self._terms()
        with np.errstate(divide="ignore"):
            logw = np.log(np.array([w for _, w in terms], dtype=np.float64))
        vmf = [i for i, (p, _) in enumerate(terms) if isinstance(p, VonMisesFisher)]
        if len(vmf) == len(terms):  # vMF terms only: the vMF-mixture target, with the arrays it has always had
            mu = _as_f64([p.mu for p, _ in terms])
            logc = _as_f64([p._log_const() for p, _ in terms]) + logw
            return _lib.VMF_MIXTURE, self.d, len(terms), 0.0, (mu, _as_f64(logc), None, None)
        # GSSS_MIXTURE: the vMF terms as one vMF-mixture component (their weights inside logc), the others one each
        comps, cw = [], []
        if vmf:
            mu = _as_f64([terms[i][0].mu for i in vmf])
            logc = _as_f64([terms[i][0]._log_const() for i in vmf]) + logw[vmf]
            comps.append((_lib.VMF_MIXTURE, self.d, len(vmf), 0.0, (mu, _as_f64(logc), None, None)))
            cw.append(0.0)
        for (p, _), lw in zip(terms, logw):
            if not isinstance(p, VonMisesFisher):
                comps.append(tuple(p._pack()[:5]))
                cw.append(lw)
        return _lib.MIXTURE, self.d, len(comps), 0.0, (), {"components": comps, "log_weights": _as_f64(cw)}

    @counted
    def log_prob(self, x):
        if self._marginal:
            with np.errstate(divide="ignore"):
                return logsumexp(np.stack([p.log_prob(x) for p in self.pdfs], axis=-1) + np.log(self.weights), axis=-1)
        return self._log_prob_device(x)

    @counted
    def gradient(self, x):
        """The softmax-weighted sum of the components' gradients (distributions.py:223-227), on the device."""
        if self._marginal:
            return _HostDensity._pack(self)
        return self._gradient_device(x)


class TargetBatch(Distribution):
    """M targets of one family and one shape, sampled in ONE launch: target t owns the contiguous block of chains
    [t m, (t + 1) m) in global chain ids, m = chains per target (the sampler derives it as n_chains / M; initial states are
    target-major).  The chains are those of M separate samplers, each on member t alone with the same seed and
    chain_offset = t m, bit for bit.

    Members: all `VonMisesFisher` / `MixtureModel` of vMF terms with the same number of terms K, or all `Bingham` /
    `BinghamFisher` (all with or all without b; `Uniform(d)` is a Bingham with A = 0), of one dimension.  A batch whose members
    are all diagonal-A Bingham runs the diagonal fast kernels, a batch that mixes diagonal and dense A the dense ones.
    Samplers: the two slice samplers on the library (Philox) stream; the Metropolis-Hastings / HMC classes, rng='numpy',
    replay and running statistics are refused.  `log_prob` / `gradient` take (M, n, d) and return (M, n) / (M, n, d): every
    member at its own rows, in one launch.  Editing a member's parameters re-uploads the batch, as for MixtureModel."""

    def __init__(self, pdfs):
        self.pdfs = list(pdfs)
        if not self.pdfs:
            raise TypeError("a target batch needs at least one member")
        packs = self._member_packs()
        kind, d, k = packs[0][:3]
        for i, (mk, md, mkk, _, arrays) in enumerate(packs):
            if mk != kind:
                raise TypeError(f"the members of a target batch are of one family: member 0 is a {self._family(kind)}, "
                                f"member {i} a {self._family(mk)}")
            if md != d:
                raise ValueError(f"the members of a target batch share the dimension: member 0 has d={d}, member {i} d={md}")
            if kind == _lib.VMF_MIXTURE and mkk != k:
                raise ValueError(f"the vMF mixtures of a target batch share the number of terms: member 0 has K={k}, "
                                 f"member {i} K={mkk}")
            if kind == _lib.BINGHAM and (arrays[0] is None) != (packs[0][4][0] is None):
                raise ValueError("the Bingham members of a target batch all have a linear term b (BinghamFisher) or none has: "
                                 f"member 0 and member {i} differ")

    @classmethod
    def tempered(cls, pdf, betas):
        """The ladder of one density for replica exchange (`sampler.exchange`, `advance(exchange=)`): member r is `pdf` at inverse
        temperature betas[r], betas descending from 1 -- the coldest member, the density itself, first.  A list of densities
        gives their ladders one behind the other (ladder-major: G R members, ladder g the members [g R, (g + 1) R)).

          Bingham(A)            -> Bingham(beta A)              an exact power
          BinghamFisher(A, b)   -> BinghamFisher(beta A, beta b) an exact power
          VonMisesFisher(mu)    -> VonMisesFisher(beta mu)       an exact power (kappa = |mu| scales)
          MixtureModel of vMF   -> the same weights, every term's mu scaled by beta

        The last is a LADDER, NOT A POWER: p^beta of a mixture is no mixture, while the members of a batch must be of one family.
        The exchange is exact all the same: a swap between members a and b is accepted with their own densities,
        alpha = p_a(x_b) p_b(x_a) / (p_a(x_a) p_b(x_b)), which leaves the product law of the batch invariant whatever the
        members are; the ladder only has to be flat enough at its hot end and close enough from rung to rung.  Any other class
        raises a TypeError.  The result carries `ladder` = len(betas) and `betas`."""
        pdfs = list(pdf) if isinstance(pdf, (list, tuple)) else [pdf]
        betas = np.array(betas, dtype=np.float64)
        if betas.ndim != 1 or len(betas) < 2 or betas[0] != 1.0 or np.any(np.diff(betas) >= 0) or betas[-1] < 0 or not np.all(np.isfinite(betas)):
            raise ValueError("betas are at least two inverse temperatures, strictly descending from 1 and not below 0")
        if not pdfs:
            raise TypeError("a target batch needs at least one member")
        members = []
        for p in pdfs:
            for beta in betas:
                if type(p) is BinghamFisher:
                    members.append(BinghamFisher(beta * p.A, beta * p.b))
                elif type(p) is Bingham:
                    members.append(Bingham(beta * p.A))
                elif type(p) is VonMisesFisher:
                    members.append(VonMisesFisher(beta * p.mu))
                elif type(p) is MixtureModel and not p._marginal and all(type(q) is VonMisesFisher for q, _ in p._terms()):
                    terms = p._terms()
                    members.append(MixtureModel([VonMisesFisher(beta * q.mu) for q, _ in terms], [w for _, w in terms]))
                elif type(p) is MixtureModel:
                    raise TypeError("a MixtureModel with other than VonMisesFisher terms has no tempered ladder: ladders are built "
                                    "of Bingham, BinghamFisher, VonMisesFisher and MixtureModel of vMF terms")
                else:
                    raise TypeError(f"{type(p).__name__} has no tempered ladder: ladders are built of Bingham, BinghamFisher, "
                                    "VonMisesFisher and MixtureModel of vMF terms")
        batch = cls(members)
        batch.ladder, batch.betas = len(betas), betas
        return batch

    @staticmethod
    def _family(kind):
        return {_lib.VMF_MIXTURE: "vMF mixture", _lib.BINGHAM: "Bingham target"}.get(kind, f"target of kind {kind}")

    def _member_packs(self):
        packs = []
        for i, p in enumerate(self.pdfs):
            if isinstance(p, TargetBatch):
                raise TypeError(f"member {i}: a TargetBatch is not a member of a target batch (concatenate the members instead)")
            if getattr(p, "_device_source", False):
                raise TypeError(f"member {i}: a DeviceDistribution (user target) is not built as a batch member")
            if not isinstance(p, Distribution):
                raise TypeError(f"member {i}: {type(p).__name__} is not a device target")
            if isinstance(p, _HostDensity) or (isinstance(p, MixtureModel) and p._marginal):
                raise TypeError(f"member {i}: {type(p).__name__} is a host-side density, not a device target")
            if not isinstance(p, (VonMisesFisher, MixtureModel, Bingham)):
                raise TypeError(f"member {i}: {type(p).__name__} is not built as a batch member: members are VonMisesFisher, "
                                "MixtureModel of vMF terms, Bingham and BinghamFisher")
            pack = p._pack()
            if pack[0] not in (_lib.VMF_MIXTURE, _lib.BINGHAM):
                raise TypeError(f"member {i}: a MixtureModel with other than vMF terms (GSSS_MIXTURE) is not built as a batch "
                                "member: members are VonMisesFisher, MixtureModel of vMF terms, Bingham and BinghamFisher")
            packs.append(tuple(pack[:5]))
        return packs

    def __len__(self):
        return len(self.pdfs)

    @property
    def d(self):
        return self.pdfs[0].d

    def _pack(self, chains_per_target=1):
        """The first member's (kind, d, k, kappa) -- the shape every member has -- and the members' own packs, in order."""
        packs = self._member_packs()
        kind, d, k, kappa = packs[0][:4]
        return kind, d, k, kappa, (), {"batch": packs, "chains_per_target": int(chains_per_target)}

    @staticmethod
    def _device_key(packed):
        kind, d, k, kappa = packed[:4]
        extra = packed[5]  # every member's parameter bytes: editing pdfs[t].A re-uploads
        return (("batch", kind, d, k, kappa, extra["chains_per_target"]) +
                tuple((m[:4],) + tuple(a.tobytes() if a is not None else None for a in m[4]) for m in extra["batch"]))

    def _device_target(self, device=None, chains_per_target=1):
        """The handle carries the chains per target (gsss_target_create_batch): one device copy per (device, m)."""
        dev = _device_index(device)
        packed = self._pack(chains_per_target)
        kind, d, k, kappa, arrays, extra = packed
        key = self._device_key(packed)
        cache = self.__dict__.setdefault("_targets", {})
        hit = cache.get((dev, int(chains_per_target)))
        if hit is None or hit[0] != key:
            cache[(dev, int(chains_per_target))] = (key, _DeviceTarget(arrays, kind, d, k, kappa, dev, extra))
        return cache[(dev, int(chains_per_target))][1]

    def launch_plan(self, chains_per_target):
        """How a fast-mode launch of the whole batch with `chains_per_target` chains each is laid out on the chip
        (gsss_batch_plan; no device needed): the chains a workgroup takes, the most targets it stages, the grid, and the share of
        the launched lanes that carry a chain.  Small m is packed: a workgroup takes a run of consecutive chains and serves every
        target the run touches.  ValueError where the batch has no fast kernel."""
        kind, d, k = self._pack()[:3]
        has_b = int(kind == _lib.BINGHAM and self._member_packs()[0][4][0] is not None)
        cpw, tpw, grid, use = C.c_int32(), C.c_int32(), C.c_int64(), C.c_double()
        _lib.check(_lib.load().gsss_batch_plan(kind, d, k, has_b, len(self.pdfs), int(chains_per_target), C.byref(cpw), C.byref(tpw),
                                               C.byref(grid), C.byref(use)))
        return {"chains_per_workgroup": cpw.value, "targets_per_workgroup": tpw.value, "grid": grid.value, "lane_use": use.value}

    def mixing_directions(self):
        """The directions `summarize(mixing=True)` holds every member's draws against -- what `enable_stats` would choose for
        the member alone: -> (hop (M, d), modes (M, K, d), weights (M, K) or None), numpy arrays.  vMF and vMF-mixture members:
        modes = the terms' mu (`MixtureModel._modes()`), weights = the member's, hop = its first mode.  Bingham and
        BinghamFisher members: hop = `.mode`, no modes (K = 0) and no weights."""
        if not isinstance(self.pdfs[0], Bingham):      # (the members are of one family)
            modes = np.array([[p.mu] if isinstance(p, VonMisesFisher) else p._modes() for p in self.pdfs], dtype=np.float64)
            weights = np.array([[1.0] if isinstance(p, VonMisesFisher) else [w for _, w in p._terms()] for p in self.pdfs],
                               dtype=np.float64)
            return modes[:, 0, :].copy(), modes, weights
        hop = np.array([p.mode for p in self.pdfs], dtype=np.float64)
        return hop, np.zeros((len(self.pdfs), 0, self.d)), None

    def hot_log_z(self, ladder=None):
        """Per ladder of `ladder` consecutive members (None: the `ladder` set by `tempered`), log of the integral of
        exp(log_prob) of the HOTTEST member (the ladder's last) over the sphere IF that member's log-density is constant in x,
        else NaN: -> (G,) numpy.  Constancy is decided from the parameters, not by sampling: a Bingham / BinghamFisher member
        with A = 0 (and b = 0), a vMF or vMF-mixture member whose every mu = 0 -- what `tempered` gives for beta = 0.  The value
        is log_prob(e_0) + log(2 pi^{d/2} / Gamma(d/2)), the constant plus the log area of the sphere: what `summarize(log_z=)`
        adds to the ladder's sums of ratios to give log Z of every rung."""
        import math
        R = getattr(self, "ladder", None) if ladder is None else int(ladder)
        if R is None:
            raise ValueError("this batch carries no ladder (TargetBatch.tempered sets one): pass ladder=R")
        M, d = len(self.pdfs), self.d
        if R < 2 or M % R:
            raise ValueError(f"the {M} targets of the batch are no run of whole ladders of {R} members (ladder >= 2)")
        log_area = math.log(2.0) + 0.5 * d * math.log(math.pi) - math.lgamma(0.5 * d)
        out = np.full(M // R, np.nan)
        for g in range(M // R):                                   # (the hottest members alone are looked at, and packed if flat)
            p = self.pdfs[g * R + R - 1]
            if isinstance(p, Bingham):
                if not np.any(p.A) and not np.any(getattr(p, "b", 0.0)):
                    out[g] = 0.0 + log_area                       # log_prob(e_0) = A_00 + b_0
            elif not any(np.any(q.mu) for q in ([p] if isinstance(p, VonMisesFisher) else [q for q, _ in p._terms()])):
                logc = np.asarray(p._pack()[4][1], dtype=np.float64).ravel()      # every mu = 0: log_prob = logsumexp_k logc_k
                top = logc.max()
                out[g] = top + math.log(float(np.exp(logc - top).sum())) + log_area
        return out

    def _batch_handle(self, device=None):
        """A device copy of the batch for evaluation: any cached one of the device whose parameters are current (the members'
        blobs do not depend on the chains per target), else a new one with one chain per target."""
        dev = _device_index(device)
        key = self._device_key(self._pack(1))
        for (cdev, _), (ckey, tgt) in self.__dict__.get("_targets", {}).items():
            if cdev == dev and ckey[:5] == key[:5] and ckey[6:] == key[6:]:
                return tgt
        return self._device_target(dev, 1)

    def _evaluate(self, x, grad):
        """One launch on the batch handle (gsss_batch_logprob / gsss_batch_gradient): x (M, n, d), numpy or a CUDA tensor."""
        M, d = len(self.pdfs), self.d
        what = "gradient" if grad else "log_prob"
        if isinstance(x, torch.Tensor):
            if x.ndim != 3 or x.shape[0] != M or x.shape[2] != d:
                raise ValueError(f"expected (M, n, d) input with M={M}, d={d}")
            if not x.is_cuda:
                raise ValueError(f"torch input to {what} must live on the GPU")
            xt = x.to(torch.float64).contiguous()
            n = int(xt.shape[1])
            out = torch.empty_like(xt) if grad else torch.empty((M, n), dtype=torch.float64, device=xt.device)
            if n == 0:
                return out
            dev = _device_index(xt.device)
            tgt = self._batch_handle(xt.device)
            fn = tgt.lib.gsss_batch_gradient if grad else tgt.lib.gsss_batch_logprob
            with torch.cuda.device(dev):
                _lib.check(fn(tgt.handle, xt.data_ptr(), n, out.data_ptr(), current_stream_ptr(dev)))
            return out
        x = np.asarray(x, dtype=np.float64)
        if x.ndim != 3 or x.shape[0] != M or x.shape[2] != d:
            raise ValueError(f"expected (M, n, d) input with M={M}, d={d}")
        _lib.require_device()
        dev = _device_index(None)
        return self._evaluate(torch.from_numpy(np.ascontiguousarray(x)).to(f"cuda:{dev}"), grad).cpu().numpy()

    @counted
    def log_prob(self, x):
        """x (M, n, d) -> (M, n): member t's log_prob of its own rows x[t], all members in one launch on the batch's own device
        copy (no member is uploaded); the values are the members' own, bit for bit."""
        return self._evaluate(x, False)

    @counted
    def gradient(self, x):
        """x (M, n, d) -> (M, n, d): member t's gradient (as the device evaluates its family's) at its own rows, in one launch."""
        return self._evaluate(x, True)


class Bingham(Distribution):
    """p(x) ~ exp(x^T A x) with symmetric A;  log_prob = sum((x @ A) * x)  (distributions.py:67-86)."""

    def __init__(self, A):
        A = np.array(A, dtype=np.float64)
        if A.ndim != 2 or A.shape[0] != A.shape[1] or not np.allclose(A, A.T):
            raise ValueError("A must be a symmetric square matrix")  # distributions.py:68
        self.A = A
        v, U = np.linalg.eigh(A)
        self.v, self.U = v[::-1], U[:, ::-1]  # descending, as the reference keeps them

    @property
    def d(self):
        return len(self.A)

    @property
    def mode(self):
        return self.U[:, 0]

    @property
    def max_log_prob(self):
        return self.v[0]

    def _pack(self):
        return _lib.BINGHAM, self.d, 0, 0.0, (None, None, _as_f64(self.A), None)

    @counted
    def log_prob(self, x):
        return self._log_prob_device(x)

    @counted
    def gradient(self, x):
        """2 A x (distributions.py:88-89); rows of points and device tensors go through the kernel's own evaluation."""
        if isinstance(x, torch.Tensor) or np.ndim(x) == 2:
            return self._gradient_device(x)
        return 2 * self.A @ np.asarray(x, dtype=np.float64)


class BinghamFisher(Bingham):
    """Fisher-Bingham: log_prob = x^T A x + x.b  (distributions.py:106-114)."""

    def __init__(self, A, b):
        super().__init__(A)
        b = np.array(b, dtype=np.float64)
        if b.shape != (len(self.A),):
            raise ValueError("b must have one entry per dimension")  # distributions.py:109
        self.b = b

    def _pack(self):
        return _lib.BINGHAM, self.d, 0, 0.0, (_as_f64(self.b), None, _as_f64(self.A), None)

    @counted
    def log_prob(self, x):
        return self._log_prob_device(x)

    # gradient: inherited from Bingham, 2 A x WITHOUT the linear term -- the reference's class does not override it
    # (distributions.py:106-114), and its spherical HMC therefore runs with that gradient; so does the kernel here.


class Uniform(Bingham):
    """The uniform distribution on the sphere (distributions.py:28-34): log_prob = 0.  The reference's class carries no
    dimension; to run a sampler on it give the ambient dimension, Uniform(d) -- on the device it is the Bingham target
    with A = 0."""

    def __init__(self, d=None):
        self._d = None if d is None else int(d)
        if d is not None:
            super().__init__(np.zeros((self._d, self._d)))

    @property
    def d(self):
        return self._d

    def _pack(self):
        if self._d is None:
            raise TypeError("Uniform() has no dimension: construct it as Uniform(d) to sample it on the device")
        return super()._pack()

    def log_prob(self, x):
        return 0.0

    def gradient(self, x):
        return np.zeros_like(x)


def random_bingham(d=2, vmax=None, vmin=None, eigensystem=False, seed=None):
    """Random Bingham target with the construction of distributions.py:230-258, so that the same
    seed gives the same precision matrix as the reference (e.g. scripts/bingham.py:131 uses
    d=10, vmax=30, vmin=0, eigensystem=True, seed=6982)."""
    g = np.random.default_rng(seed)
    M = g.standard_normal((d, d))
    spectrum, basis = np.linalg.eigh(M.T @ M)
    if vmin is not None:
        spectrum += vmin - spectrum.min()
    if vmax is not None:
        spectrum *= vmax / spectrum.max()
    if eigensystem:
        basis = np.eye(d)
    return Bingham((basis * spectrum) @ basis.T)


class SlerpCurve:
    """Piecewise-geodesic curve through `knots` (rows, unit vectors); spherical_curve.py:74-85."""

    def __init__(self, knots):
        self.knots = np.array(knots, dtype=np.float64)
        if self.knots.ndim != 2 or self.knots.shape[0] < 2:
            raise ValueError("need at least two knots")
        # arc lengths and the normalised arc-length parameter of the knots (spherical_curve.py:80-85)
        seg = np.arccos(np.clip(np.sum(self.knots[:-1] * self.knots[1:], axis=-1), -1, 1))
        self.theta = np.append(0.0, seg)
        self.bins = np.cumsum(self.theta) / np.sum(self.theta)
        self.widths = np.diff(self.bins)

    def __call__(self, t):
        """Points of the curve at arc-length parameters t in [0, 1] (spherical_curve.py:87-93) -- for plots; the sampler
        kernels never evaluate the curve, they project onto it."""
        t = np.atleast_1d(np.asarray(t, dtype=np.float64))
        s = self.bins
        i = np.clip(np.digitize(t, s, right=True), 1, len(self.knots) - 1)
        omega, span = self.theta[i], s[i] - s[i - 1]
        wa = np.sin(omega * (s[i] - t) / span) / np.sin(omega)
        wb = np.sin(omega * (t - s[i - 1]) / span) / np.sin(omega)
        return wa[:, None] * self.knots[i - 1] + wb[:, None] * self.knots[i]

    def find_nearest(self, point):
        """The point of the curve closest to `point` (spherical_curve.py:95-102): per segment the clipped great-arc
        projection of distance_slerp, then the first segment of least distance.  Host helper for plots and checks; on
        the sampler's path the projection lives in the kernels (CurvedVonMisesFisher.log_prob evaluates there)."""
        best, out = np.inf, None
        for a, b in zip(self.knots[:-1], self.knots[1:]):
            dist, y = distance_slerp(point, a, b)
            if dist < best:
                best, out = dist, y
        return out


def distance_slerp(x, a, b):
    """(geodesic distance from `x` to the great arc a -> b, closest point of the arc) (spherical_curve.py:10-32)."""
    x, a, b = (np.asarray(v, dtype=np.float64) for v in (x, a, b))
    arc = np.arccos(np.clip(a @ b, -1, 1))
    ax, bx = a @ x, b @ x
    t = np.clip(np.arctan2(bx - ax * np.cos(arc), ax * np.sin(arc)), 0.0, arc)
    y = (np.sin(arc - t) * a + np.sin(t) * b) / (np.sin(arc) + 1e-10)
    return np.arccos(np.clip(x @ y, -1, 1)), y


def brownian_curve(n_points=100, dimension=6, step_size=0.05, seed=1234):
    """Knots of a random walk on the sphere, the construction of spherical_curve.py:105-129
    (same seed -> same knots as the reference: scripts/curve_vMF.py:577-582)."""
    g = np.random.default_rng(seed)
    pts = np.zeros((n_points, dimension))
    z = g.standard_normal(dimension)
    pts[0] = z / (np.linalg.norm(z) + 1e-100)
    for i in range(1, n_points):
        w = pts[i - 1] + g.normal(size=dimension) * step_size
        pts[i] = w / (np.linalg.norm(w) + 1e-100)
    return pts


def constrained_brownian_curve(n_points=100, dimension=6, step_size=0.05, seed=1234):
    """Knots of a smooth walk on the sphere that keeps its heading (spherical_curve.py:132-181; the curve of
    scripts/curve_3d.py): each step turns the unit heading by `step_size` towards a random direction orthogonal to both the
    position and the heading, re-tangentialises it, and moves the point by the angle `step_size` along it.  Same seed ->
    same knots as the reference."""
    g = np.random.default_rng(seed)
    pts = np.zeros((n_points, dimension))
    z = g.standard_normal(dimension)
    pts[0] = z / (np.linalg.norm(z) + 1e-100)

    def tangential_unit(w, p):
        w = w - (w @ p) * p
        return w / np.linalg.norm(w)

    heading = tangential_unit(g.standard_normal(dimension), pts[0])
    for i in range(1, n_points):
        p = pts[i - 1]
        kick = g.standard_normal(dimension)
        kick -= (kick @ p) * p
        kick -= (kick @ heading) * heading
        heading = tangential_unit(heading + step_size * kick / np.linalg.norm(kick), p)
        pts[i] = np.cos(step_size) * p + np.sin(step_size) * heading
    return pts


class CurvedVonMisesFisher(Distribution):
    """log_prob = kappa * x . nearest_point_on_curve(x)  (distributions.py:263-275)."""

    def __init__(self, curve, kappa=100.0):
        if not hasattr(curve, "knots"):
            raise TypeError("curve must expose .knots (SlerpCurve)")
        self.curve = curve
        self.kappa = float(kappa)

    @property
    def d(self):
        return self.curve.knots.shape[-1]

    def _pack(self):
        knots = _as_f64(self.curve.knots)
        return _lib.CURVE_VMF, self.d, knots.shape[0], self.kappa, (None, None, None, knots)

    @counted
    def log_prob(self, x):
        return self._log_prob_device(x)

    @counted
    def gradient(self, x):
        """kappa * the nearest point of the curve (distributions.py:277-278), on the device."""
        return self._gradient_device(x)
