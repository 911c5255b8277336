"""Chain diagnostics with the reference's definitions, batched over chains and device-resident.

    acf, acf_fft, IAT, n_eff      geosss/utils.py:96-134
    ess_bulk                      the arviz estimator the paper's relative ESS comes from (scripts/bingham.py:43-57)
    distance                      geosss/sphere.py:64-68
    hopping_frequency             scripts/bingham.py:23-25
    mode_occupancy, mode_kl       scripts/vMF_diagnostics.py:335-342

Inputs may be numpy arrays or torch tensors (CPU or GPU); the time axis is the last-but-one for
sample arrays (..., n_draws, d) and the last one for scalar series (..., n_draws), so a whole
(chains, draws, dims) ensemble from `sampler.sample(..., as_tensor=True)` is analysed without leaving
the GPU.  One scalar series gives the reference's scalar.
"""
import numpy as np
import torch

from . import _lib
from .sphere import current_stream_ptr

__all__ = ["acf", "acf_fft", "IAT", "n_eff", "distance", "hopping_frequency", "mode_occupancy", "mode_kl", "from_running",
           "iat_from_acf", "ess_bulk", "ess_between_chains", "target_moments", "from_target_moments", "TargetMoments",
           "target_log_prob", "scalar_moments", "from_scalar_moments", "best_draw", "target_autocov", "from_target_autocov",
           "target_mixing", "from_target_mixing", "target_marginals", "from_target_marginals", "marginal_quantile", "ring_plan"]


def _t(x):
    return x if isinstance(x, torch.Tensor) else torch.as_tensor(np.asarray(x, dtype=np.float64))


def _back(y, like):
    if isinstance(like, torch.Tensor):
        return y
    y = y.cpu().numpy()
    return y.item() if y.ndim == 0 else y


def acf_fft(x):
    """Autocorrelation by the convolution theorem, lags 0 .. n//2-1 (utils.py:113-116), along the last axis."""
    t = _t(x).to(torch.float64)
    n = t.shape[-1]
    z = (t - t.mean(-1, keepdim=True)) / t.std(-1, unbiased=False, keepdim=True)
    f = torch.fft.rfft(z, dim=-1)
    # like np.fft.irfft without `n`: the inverse has 2*(len(f)-1) points (n-1 for odd n), as in the reference
    ac = torch.fft.irfft(f.conj() * f, n=2 * (f.shape[-1] - 1), dim=-1)[..., : n // 2] / n
    return _back(ac, x)


def acf(x, n_max=None):
    """Direct autocorrelation estimate for lags < n_max (utils.py:96-110), along the last axis."""
    t = _t(x).to(torch.float64)
    n = t.shape[-1]
    n_max = n_max or n // 2
    z = t - t.mean(-1, keepdim=True)
    ac = torch.stack([(z[..., i:] * z[..., : n - i]).mean(-1) for i in range(n_max)], dim=-1)
    return _back(ac / ac[..., :1], x)


def IAT(x, n=None):
    """Integrated autocorrelation time by the heuristic of utils.py:119-131: adjacent-pair sums of the
    autocorrelation from lag 2, truncated at the first negative pair."""
    ac = _t(acf_fft(_t(x)))
    if n:
        ac = ac[..., :n]
    m = ac.shape[-1]
    tail = ac[..., 2:-1] if m % 2 != 0 else ac[..., 2:]
    sums = tail.reshape(*tail.shape[:-1], -1, 2).sum(-1)
    neg = sums < 0
    has = neg.any(-1)
    first = torch.argmax(neg.to(torch.int64), dim=-1)                 # index of the first negative pair
    L = torch.where(has, 1 + 2 * first, torch.full_like(first, m - 1))
    lag = torch.arange(m, device=ac.device)
    keep = (lag >= 1) & (lag <= L.unsqueeze(-1))
    s = (ac * keep).sum(-1)
    return _back(1.0 + torch.clamp(2.0 * s, min=0.0), x)


def n_eff(x, n=None):
    """Effective sample size len(x) / IAT(x) (utils.py:132-134)."""
    t = _t(x)
    return _back(t.shape[-1] / _t(IAT(t, n)), x)


def distance(x, y):
    """Great-circle distance arccos(clip(x.y, -1, 1)) (sphere.py:64-68)."""
    a, b = _t(x).to(torch.float64), _t(y).to(torch.float64)
    return _back(torch.arccos(torch.clamp((a * b).sum(-1), -1.0, 1.0)), x)


def hopping_frequency(samples, mode):
    """Fraction of consecutive draws on opposite sides of the mode's equator (scripts/bingham.py:23-25);
    samples (..., n_draws, d)."""
    s = _t(samples).to(torch.float64)
    side = torch.sign(s @ _t(mode).to(s))
    return _back((side[..., 1:] != side[..., :-1]).to(torch.float64).mean(-1), samples)


def mode_occupancy(samples, modes):
    """Share of draws whose nearest mode (largest x.mu_k) is k; samples (..., d) flattened."""
    s = _t(samples).to(torch.float64).reshape(-1, _t(samples).shape[-1])
    k = torch.argmax(s @ _t(modes).to(s).T, dim=1)
    occ = torch.bincount(k, minlength=len(modes)).to(torch.float64) / len(k)
    return _back(occ, samples)


def mode_kl(occupancy, weights):
    """KL(occupancy || weights) with the reference's 1e-100 floor for empty modes."""
    p = _t(occupancy).to(torch.float64)
    p = torch.where(p > 0, p, torch.full_like(p, 1e-100))
    w = _t(weights).to(p)
    return _back((p * torch.log(p / w)).sum(), occupancy)


def saff_sphere(n=1000):
    """n points spread over S^2 along the Saff-Kuijlaars spiral, as the reference's evaluation notebooks lay out their
    histogram cells (scripts/visualize_curve_vMF.ipynb `saff_sphere`): heights h_k equally spaced in [-1, 1], azimuth
    advancing by 3.6 / sqrt(n (1 - h_k^2)); the two poles at azimuth 0."""
    h = np.linspace(-1.0, 1.0, n)
    phi = np.zeros(n)
    phi[1:-1] = np.cumsum(3.6 / np.sqrt(n * (1.0 - h[1:-1] ** 2)))   # azimuth of point k: the increments of points 1 .. k
    theta = np.arccos(h)
    return np.stack([np.cos(phi) * np.sin(theta), np.sin(phi) * np.sin(theta), np.cos(theta)], axis=1)


def grid_kl(pdf, samples, n_saff=1500, eps=1e-12):
    """KL divergence between a target on S^2 and the draws, the estimator of the reference's curve evaluation
    (scripts/visualize_curve_vMF.ipynb `calc_kld`): p = the target's probabilities on the `n_saff` spiral points
    (normalised over them), q = the share of draws whose nearest spiral point is each cell (+ eps), summed over the
    cells with p > eps.  samples: (draws, 3) or (chains, draws, 3) -> one value per chain.  Runs where the draws live."""
    s = _t(samples).to(torch.float64)
    single = s.dim() == 2
    if single:
        s = s[None]
    grid_np = saff_sphere(n_saff)
    logp = torch.as_tensor(np.asarray(pdf.log_prob(grid_np), dtype=np.float64), device=s.device)
    p = torch.exp(logp - torch.logsumexp(logp, 0))
    grid = torch.as_tensor(grid_np, device=s.device)
    out = []
    for chain in s:                                    # nearest spiral point = largest dot product on the unit sphere
        cell = torch.cat([torch.argmax(c @ grid.T, dim=1) for c in chain.split(1 << 18)])
        q = torch.bincount(cell, minlength=n_saff).to(torch.float64) / len(cell) + eps
        m = p > eps
        out.append((p[m] * (torch.log(p[m]) - torch.log(q[m]))).sum())
    kl = torch.stack(out)
    return _back(kl[0] if single else kl, samples)


def pair_sum_went_negative(ac):
    """Whether the pair-sum rule of utils.py:119-131 found its stopping point inside the given lags (per series)."""
    ac = _t(ac)
    m = ac.shape[-1]
    tail = ac[..., 2:-1] if m % 2 != 0 else ac[..., 2:]
    return (tail.reshape(*tail.shape[:-1], -1, 2).sum(-1) < 0).any(-1)


def iat_from_acf(ac):
    """The IAT heuristic of utils.py:119-131 applied to a given autocorrelation (lags 0 .. m-1 along the last
    axis): adjacent-pair sums from lag 2, truncated at the first negative pair."""
    ac = _t(ac)
    m = ac.shape[-1]
    tail = ac[..., 2:-1] if m % 2 != 0 else ac[..., 2:]
    sums = tail.reshape(*tail.shape[:-1], -1, 2).sum(-1)
    neg = sums < 0
    has = neg.any(-1)
    first = torch.argmax(neg.to(torch.int64), dim=-1)
    L = torch.where(has, 1 + 2 * first, torch.full_like(first, m - 1))
    lag = torch.arange(m, device=ac.device)
    keep = (lag >= 1) & (lag <= L.unsqueeze(-1))
    return 1.0 + torch.clamp(2.0 * (ac * keep).sum(-1), min=0.0)


def from_running(acc, d, n_modes, n_lags, second_moment=True):
    """Diagnostics from the running statistics the sampler kernels accumulate (include/gsss.h: gsss_run_args.stats_dev;
    rows x chains).  Per chain, with the reference's definitions on the retained series:
        n, mean (d), second_moment (d, d; absent when the rows were left out: GSSS_STATS_NO_SECOND_MOMENT),
        geodesic_step (sphere.distance of consecutive draws, mean),
        hopping_frequency (scripts/bingham.py:23-25), mode_occupancy (K; scripts/vMF_diagnostics.py:335-342),
        acf (lags 0 .. L of the projection, the direct estimator utils.acf, utils.py:96-110 -- identical to
        diagnostics.acf(series, n_max=L+1)), iat / n_eff (pair-sum heuristic of utils.py:119-134 on that acf),
        iat_truncated (True where no adjacent pair of the L lags went negative: the sum stopped at the window's end and
        the IAT is a LOWER bound -- raise `lags` or thin more)."""
    acc = _t(acc).to(torch.float64)
    T = d * (d + 1) // 2 if second_moment else 0
    r_sum, r_xx = 1 + d, 1 + 2 * d
    r_dist = r_xx + T
    r_hop, r_mode = r_dist + 1, r_dist + 2
    r_p = r_mode + n_modes
    r_lag, r_ring, r_head = r_p + 2, r_p + 2 + n_lags, r_p + 2 + 2 * n_lags
    n = acc[0]
    out = {"n": n, "mean": (acc[r_sum:r_sum + d] / n).T}
    if second_moment:
        sm = torch.zeros((acc.shape[1], d, d), dtype=torch.float64, device=acc.device)
        iu = torch.triu_indices(d, d)
        sm[:, iu[0], iu[1]] = (acc[r_xx:r_xx + T] / n).T
        sm[:, iu[1], iu[0]] = (acc[r_xx:r_xx + T] / n).T
        out["second_moment"] = sm
    out["geodesic_step"] = acc[r_dist] / (n - 1)
    out["hopping_frequency"] = acc[r_hop] / (n - 1)
    if n_modes:
        out["mode_occupancy"] = (acc[r_mode:r_mode + n_modes] / n).T
    out["proj_mean"] = acc[r_p] / n                                            # mean and (biased) variance of p = x . w per chain
    out["proj_var"] = acc[r_p + 1] / n - out["proj_mean"] ** 2
    if n_lags:
        L = n_lags
        if bool((n <= L).any()):
            raise ValueError("the autocorrelation needs more than `lags` retained draws per chain")
        sp, spp = acc[r_p], acc[r_p + 1]
        mu = sp / n
        lag = torch.arange(1, L + 1, device=acc.device, dtype=torch.float64)[:, None]
        head = torch.cumsum(acc[r_head:r_head + L], dim=0)                    # sum of the first l values
        # the last l values: ring slot (n - j) mod L holds p_{n-j}, j = 1 .. L
        j = torch.arange(1, L + 1, device=acc.device)[:, None]
        slot = torch.remainder(n.to(torch.int64)[None, :] - j, L)
        tail = torch.cumsum(torch.gather(acc[r_ring:r_ring + L], 0, slot), dim=0)
        c = acc[r_lag:r_lag + L]
        cov = (c - mu * ((sp - head) + (sp - tail)) + (n - lag) * mu * mu) / (n - lag)
        var = (spp - n * mu * mu) / n
        ac = torch.cat([torch.ones_like(var)[None], cov / var], dim=0).T     # (chains, L + 1)
        out["acf"] = ac
        out["iat"] = iat_from_acf(ac)
        out["n_eff"] = n / out["iat"]
        out["iat_truncated"] = ~pair_sum_went_negative(ac)
    return out


def ess_between_chains(chain_means, n, chain_vars):
    """Integrated autocorrelation time and effective sample size of a scalar quantity from MANY independent stationary chains,
    with no lag window at all: for a stationary chain Var(mean of n draws) = Var(x) tau_n / n with
    tau_n = 1 + 2 sum_{k<n} (1 - k/n) rho_k -> tau, so over C chains of n draws each

        tau = n Var_c(mean_c) / Var(x),      ESS per chain = n / tau = Var(x) / Var_c(mean_c),

    Var(x) = the pooled variance of all draws = mean_c(within-chain variance) + Var_c(mean_c) (law of total variance).
    Inputs per chain: the mean, the number of draws and the (biased, 1/n) variance of the series -- `proj_mean`, `n`,
    `proj_var` of `from_running`, i.e. the sums the sampler kernels already keep.  What the windowed estimators
    (geosss/utils.py:109-134 IAT / n_eff on a truncated autocorrelation) can only bound from below when the chain mixes
    slower than the window, this measures -- to a relative standard error sqrt(2 / (C - 1)) -- provided the chains ARE
    independent and stationary (start them from draws of the target, or burn in several tau) and n >> tau (the finite-n
    factor (1 - k/n) biases tau low by ~ tau / n otherwise).  Returns a dict of floats:
    tau (in retained draws), ess_per_chain, ess_total, rel_se, n, chains."""
    m, v = _t(chain_means).to(torch.float64).reshape(-1), _t(chain_vars).to(torch.float64).reshape(-1)
    nn = _t(n).to(torch.float64).reshape(-1)
    if m.numel() < 2:
        raise ValueError("the between-chain estimator needs at least two chains")
    if float(nn.max() - nn.min()) != 0.0:
        raise ValueError("the between-chain estimator takes chains of equal length")
    n_draws = float(nn[0])
    between = float(m.var(unbiased=True))
    total = float(v.mean()) + between
    if not between > 0.0 or not total > 0.0:
        return {"tau": float("nan"), "ess_per_chain": float("nan"), "ess_total": float("nan"), "rel_se": float("nan"),
                "n": n_draws, "chains": int(m.numel())}
    tau = n_draws * between / total
    return {"tau": tau, "ess_per_chain": n_draws / tau, "ess_total": m.numel() * n_draws / tau,
            "rel_se": float(np.sqrt(2.0 / (m.numel() - 1))), "n": n_draws, "chains": int(m.numel())}


def _accumulator(name, t, shape, like, of="x", dtype=torch.float64):
    """The accumulator t, or zeros for None; ValueError unless it is contiguous, of this shape and dtype, on the device of `like`."""
    if t is None:
        return torch.zeros(shape, dtype=dtype, device=like.device)
    if (not isinstance(t, torch.Tensor) or tuple(t.shape) != tuple(shape) or t.dtype != dtype or t.device != like.device
            or not t.is_contiguous()):
        raise ValueError(f"{name} must be a contiguous {str(dtype)[6:]} tensor {tuple(shape)} on the device of {of}")
    return t


def _chains_per_target(chains_per_target, n):
    m = int(chains_per_target)
    if m < 1 or n % m:
        raise ValueError(f"the number of chains ({n}) must be a multiple of chains_per_target ({chains_per_target})")
    return m


def _device_index(t):
    return t.device.index if t.device.index is not None else torch.cuda.current_device()


def _moments_form(d, second_moment):
    """(keep the full triangle?, accumulator rows per target) -- the rows of gsss_moments_rows."""
    full = d <= 16 if second_moment is None else bool(second_moment)
    if full and d > 16:
        raise ValueError("the full second-moment triangle is kept for d <= 16: pass second_moment=False for the diagonal")
    return full, 1 + d + (d * (d + 1) // 2 if full else d)


def target_moments(x, chains_per_target, *, chain_major=False, second_moment=None, acc=None, chain_sum=None):
    """Per-target sums of a block of draws on the device, in one pass and without atomics (gsss_target_moments, include/gsss.h).

    x: a CUDA float64 tensor, component-major (R, d, n) -- what `advance(..., thin=t)` returns -- or, with chain_major=True,
    (n, R, d) -- what `sample(..., as_tensor=True)` returns; a slice of rows of such an array is taken where it lies.  Target t
    owns the chains [t m, (t + 1) m), m = chains_per_target.  Returns the accumulator (M, rows), M = n / m: row 0 the count of
    draws, rows 1 .. d the sums of x_j, then the d (d + 1) / 2 sums of x_i x_j (i <= j, row-major; second_moment=None keeps them
    for d <= 16) or, with second_moment=False, the d sums of x_j^2.  `acc` continues an earlier accumulator (added to, returned);
    `chain_sum`, a (d, n) tensor, has every chain's sum of its R draws added to it."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64 or x.ndim != 3:
        raise ValueError("x must be a CUDA float64 tensor (R, d, n), or (n, R, d) with chain_major=True")
    if chain_major:
        n, R, d = (int(v) for v in x.shape)
        if n * R and not (x.stride(2) == 1 and x.stride(1) == d and x.stride(0) % d == 0 and x.stride(0) >= R * d):
            x = x.contiguous()
        chain_rows = int(x.stride(0)) // d if n * R else max(R, 1)
    else:
        R, d, n = (int(v) for v in x.shape)
        x, chain_rows = x.contiguous(), 0
    full, rows = _moments_form(d, second_moment)
    m = _chains_per_target(chains_per_target, n)
    acc = _accumulator("acc", acc, (n // m, rows), x)
    if chain_sum is not None:
        _accumulator("chain_sum", chain_sum, (d, n), x)
    if R == 0 or n == 0:
        return acc
    dev = _device_index(x)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsss_target_moments(x.data_ptr(), R, n, d, chain_rows, m, 0 if full else _lib.MOMENTS_DIAG,
                                                   acc.data_ptr(), None if chain_sum is None else chain_sum.data_ptr(), dev,
                                                   current_stream_ptr(dev)))
    return acc


def from_target_moments(acc, d, *, chain_sum=None, chains_per_target=None, second_moment=True):
    """Per-target summaries from the accumulators of `target_moments` / `Sampler.summarize`; every entry has the leading axis M.
    With N = acc[:, 0] draws per target, S_j = sum x_j and Q_ij = sum x_i x_j:

        n = N,  mean_j = S_j / N,  second_moment_ij = Q_ij / N (symmetric; second_moment=False: second_moment_diag_j = Q_jj / N),
        cov = second_moment - mean mean^T,  var_j = Q_jj / N - mean_j^2 (biased, 1 / N),
        resultant_length = |mean|,  mean_direction = mean / |mean|.

    With chain_sum (d, n) and m = chains_per_target, the chains of a target are compared, per coordinate j.  A chain has
    r = N / m draws and the mean c = chain_sum / r; over the m chains of the target

        between_j = (sum c^2 - (sum c)^2 / m) / (m - 1)        the unbiased variance of the chain means,
        within_j  = Q_jj / N - (sum c^2) / m                    the mean of the chains' own (biased, 1 / r) variances,
        rhat_j    = sqrt((within_j + between_j) / (within_j r / (r - 1)))     Gelman-Rubin: var+ = (r - 1) / r W + B / r over W
                                                                with W = within r / (r - 1) and B / r = between,
        ess_between_j = (within_j + between_j) / between_j      ess_between_chains' "ess_per_chain": pooled variance over the
                                                                variance of the chain means.

    On CUDA tensors sum c and sum c^2 come from the moments kernel itself, run on the one row of chain means; CPU tensors take
    the same sums with torch."""
    acc = _t(acc).to(torch.float64)
    M = acc.shape[0]
    n = acc[:, 0]
    mean = acc[:, 1:1 + d] / n[:, None]
    out = {"n": n, "mean": mean}
    if second_moment:
        T = d * (d + 1) // 2
        iu = torch.triu_indices(d, d, device=acc.device)
        q = acc[:, 1 + d:1 + d + T] / n[:, None]
        sm = torch.zeros((M, d, d), dtype=torch.float64, device=acc.device)
        sm[:, iu[0], iu[1]] = q
        sm[:, iu[1], iu[0]] = q
        out["second_moment"] = sm
        out["cov"] = sm - mean[:, :, None] * mean[:, None, :]
        qd = torch.diagonal(sm, dim1=1, dim2=2)
    else:
        qd = acc[:, 1 + d:1 + 2 * d] / n[:, None]
        out["second_moment_diag"] = qd
    out["var"] = qd - mean * mean
    rl = torch.linalg.norm(mean, dim=1)
    out["resultant_length"] = rl
    out["mean_direction"] = mean / rl[:, None]
    if chain_sum is None:
        return out
    if chains_per_target is None:
        raise ValueError("chain_sum needs chains_per_target")
    m = int(chains_per_target)
    cs = _t(chain_sum).to(torch.float64)
    if cs.ndim != 2 or cs.shape[0] != d or cs.shape[1] != M * m:
        raise ValueError(f"chain_sum must be (d, n) = ({d}, {M * m})")
    r = n / m                                                        # draws per chain
    cm = (cs.reshape(d, M, m) / r[None, :, None]).reshape(1, d, M * m)
    if cm.is_cuda:
        a2 = target_moments(cm, m, second_moment=False)               # the same kernel on the row of chain means
        s1, s2 = a2[:, 1:1 + d], a2[:, 1 + d:1 + 2 * d]
    else:
        c3 = cm.reshape(d, M, m)
        s1, s2 = c3.sum(-1).T, (c3 * c3).sum(-1).T
    between = (s2 - s1 * s1 / m) / (m - 1) if m > 1 else torch.full_like(s1, float("nan"))
    within = qd - s2 / m
    out["between"], out["within"] = between, within
    out["rhat"] = torch.sqrt((within + between) / (within * (r / (r - 1))[:, None]))
    out["ess_between"] = (within + between) / between
    return out


def target_log_prob(batch, x, *, chain_major=False, target0=0):
    """log_prob of a block of draws under the targets of a TargetBatch that own them, in one launch and where the draws lie
    (gsss_batch_logprob_draws, include/gsss.h).

    x: a CUDA float64 tensor, component-major (R, d, N) -- what `advance(..., thin=t)` returns -- -> (R, N); or, with
    chain_major=True, (N, R, d) -- what `sample(..., as_tensor=True)` returns -- -> (N, R).  The block covers the targets
    target0 .. len(batch) - 1, each with the same number of chains: m = N / (len(batch) - target0), which must divide; chain c
    belongs to target target0 + c // m.  The values are the members' own `log_prob`, bit for bit."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64 or x.ndim != 3:
        raise ValueError("x must be a CUDA float64 tensor (R, d, N), or (N, R, d) with chain_major=True")
    N, R, d = (int(v) for v in (x.shape if chain_major else (x.shape[2], x.shape[0], x.shape[1])))
    M, target0 = len(batch), int(target0)
    if d != batch.d:
        raise ValueError(f"the batch's targets live in d={batch.d} (got {d})")
    if not 0 <= target0 < M:
        raise ValueError(f"target0 ({target0}) must be one of the batch's {M} targets")
    covered = M - target0
    if N < covered or N % covered:
        raise ValueError(f"the number of chains ({N}) must be a multiple of the {covered} targets covered (target0 = {target0} .. "
                         f"{M - 1}), with at least one chain each")
    m = N // covered
    out = torch.empty((N, R) if chain_major else (R, N), dtype=torch.float64, device=x.device)
    if R == 0:
        return out
    dev = _device_index(x)
    tgt = batch._device_target(x.device, chains_per_target=m)
    with torch.cuda.device(dev):
        if chain_major and target0 == 0:   # (N, R, d) is row-major (M, m R, d): every member at its own rows
            x = x.contiguous()
            _lib.check(tgt.lib.gsss_batch_logprob(tgt.handle, x.data_ptr(), m * R, out.data_ptr(), current_stream_ptr(dev)))
            return out
        xc = x.permute(1, 2, 0).contiguous() if chain_major else x.contiguous()
        oc = torch.empty((R, N), dtype=torch.float64, device=x.device) if chain_major else out
        _lib.check(tgt.lib.gsss_batch_logprob_draws(tgt.handle, xc.data_ptr(), R, N, target0, oc.data_ptr(), current_stream_ptr(dev)))
    if chain_major:
        out.copy_(oc.t())
    return out


def scalar_moments(values, chains_per_target, *, acc=None, chain_sum=None):
    """`target_moments` for one scalar per draw (gsss_scalar_moments): values (R, N), a CUDA float64 tensor, target t owning the
    chains [t m, (t + 1) m).  Returns acc (M, 3): count, sum v, sum v^2 -- `acc` continues an earlier one; `chain_sum` (N,) has
    every chain's sum of its R values added to it.  The same kernels, the same fixed summation order."""
    if not isinstance(values, torch.Tensor) or not values.is_cuda or values.dtype != torch.float64 or values.ndim != 2:
        raise ValueError("values must be a CUDA float64 tensor (R, N)")
    values = values.contiguous()
    R, N = (int(v) for v in values.shape)
    m = _chains_per_target(chains_per_target, N)
    acc = _accumulator("acc", acc, (N // m, 3), values, of="the values")
    if chain_sum is not None:
        _accumulator("chain_sum", chain_sum, (N,), values, of="the values")
    if R == 0 or N == 0:
        return acc
    dev = _device_index(values)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsss_scalar_moments(values.data_ptr(), R, N, m, acc.data_ptr(),
                                                   None if chain_sum is None else chain_sum.data_ptr(), dev, current_stream_ptr(dev)))
    return acc


def best_draw(values, chains_per_target):
    """The largest value per target of a block values (R, N), target t owning the chains [t m, (t + 1) m), and where it is:
    -> (best (M,), row (M,), chain (M,)), chain in 0 .. N - 1.  Ties go to the earliest row, then to the lowest chain (the
    first occurrence in (row, chain) order, found as the smallest index that attains the maximum: the same on every device)."""
    v = _t(values)
    R, N = (int(s) for s in v.shape)
    m = int(chains_per_target)
    M = N // m
    flat = v.reshape(R, M, m).permute(1, 0, 2).reshape(M, R * m)      # index: row m + chain of the target
    best = flat.amax(dim=1)
    pos = torch.arange(R * m, device=v.device)
    first = torch.where(flat == best[:, None], pos[None, :], R * m - 1).amin(dim=1)
    return best, first // m, torch.arange(M, device=v.device) * m + first % m


def from_scalar_moments(acc, chain_sum, chains_per_target):
    """`from_target_moments` for one scalar per draw: acc (M, 3) = count N, S = sum v, Q = sum v^2, chain_sum (M m,).  With
    r = N / m draws a chain and c = chain_sum / r the chain means:  mean = S / N,  var = Q / N - mean^2 (biased),
    between = (sum c^2 - (sum c)^2 / m) / (m - 1),  within = Q / N - (sum c^2) / m,
    rhat = sqrt((within + between) / (within r / (r - 1))),  ess_between = (within + between) / between.  CPU or CUDA tensors."""
    acc = _t(acc).to(torch.float64)
    m = int(chains_per_target)
    M = acc.shape[0]
    n = acc[:, 0]
    mean, q = acc[:, 1] / n, acc[:, 2] / n
    r = n / m
    cm = _t(chain_sum).to(torch.float64).reshape(M, m) / r[:, None]
    s1, s2 = cm.sum(-1), (cm * cm).sum(-1)
    between = (s2 - s1 * s1 / m) / (m - 1) if m > 1 else torch.full_like(s1, float("nan"))
    within = q - s2 / m
    return {"mean": mean, "var": q - mean * mean, "between": between, "within": within,
            "rhat": torch.sqrt((within + between) / (within * (r / (r - 1)))), "ess_between": (within + between) / between}


def target_autocov(x, chains_per_target, lags, *, acc=None, hist=None):
    """Per-target lagged products of a block of draws on the device, in one pass and without atomics (gsss_target_autocov,
    include/gsss.h).

    x: a CUDA float64 tensor, component-major (R, d, n) -- what `advance(..., thin=t)` returns -- or (R, n) for a scalar series.
    Target t owns the chains [t m, (t + 1) m), m = chains_per_target.  Returns the accumulator (M, d, L + 1, 3), M = n / m,
    L = lags: for every target, series j and lag l the sums over the target's chains and the rows r of
    C = x_{r,j} x_{r-l,j}, P = x_{r,j} and Q = x_{r-l,j}, a pair counting where r - l is a row of x or of `hist`.  `hist`: the up to
    `lags` rows that precede x (same trailing shape, oldest first), for a caller who streams a series block by block; `acc`
    continues an earlier accumulator (added to, returned).  -> `from_target_autocov`."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64 or x.ndim not in (2, 3):
        raise ValueError("x must be a CUDA float64 tensor (R, d, n), or (R, n) for a scalar series")
    if x.ndim == 2:
        x = x[:, None, :]
    R, d, n = (int(v) for v in x.shape)
    m, L = _chains_per_target(chains_per_target, n), int(lags)
    if not 1 <= L <= 64:
        raise ValueError(f"lags must be 1 .. 64 (got {lags})")
    M, h = n // m, 0
    if hist is not None:
        if isinstance(hist, torch.Tensor) and hist.ndim == 2:
            hist = hist[:, None, :]
        if (not isinstance(hist, torch.Tensor) or hist.ndim != 3 or tuple(hist.shape[1:]) != (d, n) or hist.dtype != torch.float64
                or hist.device != x.device or hist.shape[0] > L):
            raise ValueError(f"hist must be a float64 tensor of at most {L} rows shaped like the rows of x, on the device of x")
        h = int(hist.shape[0])
    acc = _accumulator("acc", acc, (M, d, L + 1, 3), x)
    if R == 0 or n == 0:
        return acc
    ring = torch.cat([x, hist]) if h else x.contiguous()     # the rows before row 0 of a ring are its last
    _autocov_fold(ring, 0, R, h, m, L, acc)
    return acc


def _autocov_fold(ring, first_row, n_rows, n_hist, m, lags, acc):
    """gsss_target_autocov on the rows first_row .. + n_rows of a contiguous ring (rows, d, n)."""
    rows, d, n = (int(v) for v in ring.shape)
    dev = _device_index(ring)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsss_target_autocov(ring.data_ptr(), rows, first_row, n_rows, n_hist, n, d, m, lags, acc.data_ptr(),
                                                   dev, current_stream_ptr(dev)))


def from_target_autocov(acov, chains_per_target, n):
    """Per-target within-chain autocorrelation from the accumulators of `target_autocov` / `Sampler.summarize(lags=L)`:
    acov (M, d, L + 1, 3) = (C, P, Q) per target, series and lag, m = chains_per_target chains of n draws each (n: a number or
    one per target).  With the pooled mean mu = P_0 / (m n) and k_l = m (n - l) pairs,

        cov_l = (C_l - mu (P_l + Q_l)) / k_l + mu^2,      acf_l = cov_l / cov_0      (M, d, L + 1),

    the direct estimator of `acf` (utils.py:96-110) centred on the target's pooled mean: at m = 1 it is
    `acf(series, n_max=L + 1)`.  iat (M, d): `iat_from_acf` (the pair-sum heuristic of utils.py:119-131); ess_within = m n / iat;
    iat_truncated: no adjacent pair of the L lags went negative, the sum stopped at the window's end and the IAT is a LOWER
    bound (raise `lags` or thin more).  CPU or CUDA tensors.  ValueError where n <= L."""
    acov = _t(acov).to(torch.float64)
    if acov.ndim != 4 or acov.shape[-1] != 3 or acov.shape[2] < 2:
        raise ValueError("acov must be (M, d, L + 1, 3)")
    m, L = int(chains_per_target), int(acov.shape[2]) - 1
    n = torch.as_tensor(n, dtype=torch.float64, device=acov.device).reshape(-1, 1, 1)
    if bool((n <= L).any()):
        raise ValueError("the autocorrelation needs more than `lags` retained draws per chain")
    c, p, q = acov[..., 0], acov[..., 1], acov[..., 2]
    mu = p[..., :1] / (m * n)
    k = m * (n - torch.arange(L + 1, dtype=torch.float64, device=acov.device))
    cov = (c - mu * (p + q)) / k + mu * mu
    ac = cov / cov[..., :1]
    iat = iat_from_acf(ac)
    return {"acf": ac, "iat": iat, "ess_within": m * n.reshape(-1, 1) / iat, "iat_truncated": ~pair_sum_went_negative(ac)}


def _mixing_dirs(hop, modes, M, d, device):
    """(dirs (M, 1 + K, d) contiguous float64 on `device`, K) from hop (d,) | (M, d) | None and modes (K, d) | (M, K, d) | None;
    the shared forms are broadcast, hop=None is a zero direction (no hops), modes=None K = 0."""
    def tensor(v, what):
        try:
            return _t(v).to(torch.float64)
        except (TypeError, ValueError) as e:
            raise ValueError(f"{what} must be an array of directions") from e
    h = torch.zeros((M, d), dtype=torch.float64) if hop is None else tensor(hop, "hop")
    if h.ndim == 1:
        h = h[None].expand(M, -1)
    if h.ndim != 2 or tuple(h.shape) != (M, d):
        raise ValueError(f"hop must be ({d},) or ({M}, {d}) (got {tuple(_t(hop).shape)})")
    k = torch.zeros((M, 0, d), dtype=torch.float64) if modes is None else tensor(modes, "modes")
    if k.ndim == 2:
        k = k[None].expand(M, -1, -1)
    if k.ndim != 3 or k.shape[0] != M or k.shape[2] != d:
        raise ValueError(f"modes must be (K, {d}) or ({M}, K, {d}) (got {tuple(_t(modes).shape)})")
    K = int(k.shape[1])
    if K > 16:
        raise ValueError(f"at most 16 mode directions are kept (got {K})")
    return torch.cat([h[:, None, :].to(device), k.to(device)], dim=1).contiguous(), K


def target_mixing(x, chains_per_target, *, hop=None, modes=None, transitions=False, step=None, counts=None, hist=None):
    """Per-target mixing sums of a block of draws on the device, in one pass (gsss_target_mixing, include/gsss.h), every target
    with its own directions.

    x: a CUDA float64 tensor, component-major (R, d, n) -- what `advance(..., thin=t)` returns.  Target t owns the chains
    [t m, (t + 1) m), m = chains_per_target, M = n / m.  hop: (d,) or (M, d), the direction whose equator a hop crosses (None:
    a zero direction, no hops); modes: (K, d) or (M, K, d), K <= 16 (None: K = 0).  Returns (step, counts): step (M, 2) =
    sum theta, sum theta^2 over the target's pairs of consecutive draws, theta = arccos(clip(x_r . x_{r-1}, -1, 1)); counts
    (M, 3 + K [+ K K]) int64 = draws, pairs, hops, the draws per mode (first maximum of x . mode_k, like np.argmax) and, with
    transitions=True, the pairs by [mode before][mode after].  `hist`: the one row (1, d, n) that precedes x, for a caller who
    streams a series block by block; `step` / `counts` continue earlier accumulators (added to, returned).
    -> `from_target_mixing`."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.ndim != 3:
        raise ValueError("x must be a CUDA float64 tensor (R, d, n)")
    R, d, n = (int(v) for v in x.shape)
    m = _chains_per_target(chains_per_target, n)
    if d < 2:
        raise ValueError("a point on a sphere has two coordinates at least")
    M, h = n // m, 0
    dirs, K = _mixing_dirs(hop, modes, M, d, x.device)
    if not x.is_cuda:
        raise ValueError("x must be a CUDA float64 tensor (R, d, n): the sums are taken on the device")
    rows = 3 + K + (K * K if transitions else 0)
    if hist is not None:
        if (not isinstance(hist, torch.Tensor) or hist.ndim != 3 or tuple(hist.shape[1:]) != (d, n) or hist.dtype != torch.float64
                or hist.device != x.device or hist.shape[0] > 1):
            raise ValueError("hist must be a float64 tensor of at most one row shaped like the rows of x, on the device of x")
        h = int(hist.shape[0])
    step = _accumulator("step", step, (M, 2), x)
    counts = _accumulator("counts", counts, (M, rows), x, dtype=torch.int64)
    if R == 0 or n == 0:
        return step, counts
    ring = torch.cat([x, hist]) if h else x.contiguous()     # the row before row 0 of a ring is its last
    _mixing_fold(ring, 0, R, h, m, dirs, K, transitions, step, counts)
    return step, counts


def _mixing_fold(ring, first_row, n_rows, n_hist, m, dirs, n_modes, transitions, step, counts):
    """gsss_target_mixing on the rows first_row .. + n_rows of a contiguous ring (rows, d, n)."""
    rows, d, n = (int(v) for v in ring.shape)
    dev = _device_index(ring)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsss_target_mixing(ring.data_ptr(), rows, first_row, n_rows, n_hist, n, d, m, dirs.data_ptr(), n_modes,
                                                  _lib.MIXING_TRANSITIONS if transitions else 0, step.data_ptr(), counts.data_ptr(),
                                                  dev, current_stream_ptr(dev)))


def from_target_mixing(step, counts, n_modes, *, weights=None):
    """Per-target mixing metrics from the accumulators of `target_mixing` / `Sampler.summarize(mixing=)`: step (M, 2), counts
    (M, 3 + K [+ K K]), K = n_modes.  With N draws and P pairs per target:

        geodesic_step = sum theta / P,  geodesic_step_sd = sqrt(max(sum theta^2 / P - geodesic_step^2, 0)),
        hop_frequency = hops / P,  mode_occupancy (M, K) = mode counts / N,

    and, where the transitions were counted, mode_transitions (M, K, K), every row [mode before] divided by its sum (NaN for a
    mode no pair left), and mode_switch_frequency = the share of the pairs whose two draws have different modes.  weights (K,)
    or (M, K): mode_kl (M,) = KL(mode_occupancy || weights) with `mode_kl`'s 1e-100 floor; weights without modes are refused.
    CPU or CUDA tensors."""
    step = _t(step).to(torch.float64)
    counts = _t(counts)
    K = int(n_modes)
    if step.ndim != 2 or step.shape[1] != 2 or counts.ndim != 2 or counts.shape[0] != step.shape[0]:
        raise ValueError("step must be (M, 2) and counts (M, 3 + K [+ K K])")
    if K < 0 or counts.shape[1] not in (3 + K, 3 + K + K * K):
        raise ValueError(f"counts must have 3 + K or 3 + K + K K columns for K = {K} (got {counts.shape[1]})")
    M = int(step.shape[0])
    c = counts.to(torch.float64)
    n, pairs = c[:, 0], c[:, 1]
    mean = step[:, 0] / pairs
    out = {"geodesic_step": mean,
           "geodesic_step_sd": torch.sqrt(torch.clamp(step[:, 1] / pairs - mean * mean, min=0.0)),
           "hop_frequency": c[:, 2] / pairs,
           "mode_occupancy": c[:, 3:3 + K] / n[:, None]}
    if K > 0 and counts.shape[1] == 3 + K + K * K:
        tr = c[:, 3 + K:].reshape(M, K, K)
        out["mode_transitions"] = tr / tr.sum(-1, keepdim=True)
        out["mode_switch_frequency"] = (pairs - torch.diagonal(tr, dim1=1, dim2=2).sum(-1)) / pairs
    if weights is not None:
        if K == 0:
            raise ValueError("mode_kl compares the mode occupancy with the weights: there are no modes")
        w = _t(weights).to(c)
        if w.ndim == 1:
            w = w[None].expand(M, -1)
        if tuple(w.shape) != (M, K):
            raise ValueError(f"weights must be ({K},) or ({M}, {K})")
        p = out["mode_occupancy"]
        p = torch.where(p > 0, p, torch.full_like(p, 1e-100))
        out["mode_kl"] = (p * torch.log(p / w)).sum(-1)
    return out


MARGINAL_QUANTILES = (0.025, 0.25, 0.5, 0.75, 0.975)  # what stats() reports of every marginal: median, quartiles, 95 % interval


def _marginals_plan(marginals):
    """dict(bins, directions, steps) of summarize(marginals=True | dict(..)), and the refusals that need no device."""
    if marginals is True:
        return {"bins": 64, "directions": None, "steps": False}
    if isinstance(marginals, dict) and not set(marginals) - {"bins", "directions", "steps"}:
        plan = {"bins": marginals.get("bins", 64), "directions": marginals.get("directions"),
                "steps": bool(marginals.get("steps", False))}
        _marginal_bins(plan["bins"])
        return plan
    raise ValueError("marginals must be True or a dict with the keys bins, directions, steps")


def _marginal_bins(bins):
    if isinstance(bins, bool) or not isinstance(bins, (int, np.integer)) or not 2 <= int(bins) <= 1024:
        raise ValueError(f"bins must be a whole number 2 .. 1024 (got {bins!r})")
    return int(bins)


def _marginal_shape(bins, n_dirs, steps):
    """B, after the refusals of gsss_marginal_rows."""
    B, S = _marginal_bins(bins), n_dirs + (1 if steps else 0)
    if n_dirs > 32:
        raise ValueError(f"at most 32 directions per target are kept (got {n_dirs})")
    if S == 0:
        raise ValueError("no directions and no steps: there is nothing to count")
    if S * B > 8192:
        raise ValueError(f"at most 8192 counters per target are kept ({S} series of {B} bins are {S * B})")
    return B


def _marginal_dirs(directions, M, d, device):
    """(dirs (M, P, d) contiguous float64 on `device`, P) from directions (P, d) | (M, P, d) | None: the shared form is broadcast,
    None is the d coordinate axes."""
    if directions is None:
        v = torch.eye(d, dtype=torch.float64)
    else:
        try:
            v = _t(directions).to(torch.float64)
        except (TypeError, ValueError) as e:
            raise ValueError("directions must be an array of directions") from e
    if v.ndim == 2:
        v = v[None].expand(M, -1, -1)
    if v.ndim != 3 or v.shape[0] != M or v.shape[2] != d:
        raise ValueError(f"directions must be (P, {d}) or ({M}, P, {d}) (got {tuple(_t(directions).shape)})")
    return v.to(device).contiguous(), int(v.shape[1])


def _n_marginal_dirs(directions, d):
    """P of `_marginal_dirs` without building them."""
    if directions is None:
        return d
    shape = tuple(directions.shape) if hasattr(directions, "shape") else np.shape(directions)
    return int(shape[-2]) if len(shape) >= 2 else -1


def target_marginals(x, chains_per_target, *, bins=64, directions=None, steps=False, chain_major=False, counts=None, hist=None):
    """Per-target marginal histograms of a block of draws on the device, in one pass (gsss_target_marginals, include/gsss.h),
    every target with its own directions.

    x: a CUDA float64 tensor, component-major (R, d, n) -- what `advance(..., thin=t)` returns -- or, with chain_major=True,
    (n, R, d) -- what `sample(..., as_tensor=True)` returns.  Target t owns the chains [t m, (t + 1) m), m = chains_per_target,
    M = n / m.  directions: (P, d) for every target or (M, P, d), P <= 32, unit vectors or not (None: the d coordinate axes).
    Returns counts (M, S, B) int64, B = bins (2 .. 1024), S = P + (1 if steps else 0), S B <= 8192: series p < P counts the target's
    draws by u = x . v_p over B equal bins of [-1, 1] -- bin floor((u + 1) B / 2), what falls outside in the first and the last
    bin; with steps=True series P counts its pairs of consecutive draws by theta = arccos(clip(x_r . x_{r-1}, -1, 1)) over B
    equal bins of [0, pi].  NaN is counted nowhere.  `hist`: the one row that precedes x, laid out like x ((1, d, n), chain-major
    (n, 1, d)), for a caller who streams a series block by block with steps; `counts` continues an earlier result (added to,
    returned).  -> `from_target_marginals`."""
    if not isinstance(x, torch.Tensor) or x.dtype != torch.float64 or x.ndim != 3:
        raise ValueError("x must be a CUDA float64 tensor (R, d, n), or (n, R, d) with chain_major=True")

    def rows_first(t):
        return t.permute(1, 2, 0) if chain_major else t
    R, d, n = (int(v) for v in rows_first(x).shape)
    m = _chains_per_target(chains_per_target, n)
    if d < 2:
        raise ValueError("a point on a sphere has two coordinates at least")
    M, h = n // m, 0
    dirs, P = _marginal_dirs(directions, M, d, x.device)
    B = _marginal_shape(bins, P, steps)
    if not x.is_cuda:
        raise ValueError("x must be a CUDA float64 tensor: the counts are taken on the device")
    if hist is not None:
        if (not isinstance(hist, torch.Tensor) or hist.ndim != 3 or tuple(rows_first(hist).shape[1:]) != (d, n)
                or hist.dtype != torch.float64 or hist.device != x.device or rows_first(hist).shape[0] > 1):
            raise ValueError("hist must be a float64 tensor of at most one row shaped like the rows of x, on the device of x")
        h = int(rows_first(hist).shape[0])
    counts = _accumulator("counts", counts, (M, P + (1 if steps else 0), B), x, dtype=torch.int64)
    if R == 0 or n == 0:
        return counts
    ring = torch.cat([rows_first(x), rows_first(hist)]) if h else rows_first(x).contiguous()   # the row before row 0 of a ring is its last
    _marginals_fold(ring, 0, R, h, m, dirs, B, steps, counts)
    return counts


def _marginals_fold(ring, first_row, n_rows, n_hist, m, dirs, bins, steps, counts):
    """gsss_target_marginals on the rows first_row .. + n_rows of a contiguous ring (rows, d, n)."""
    rows, d, n = (int(v) for v in ring.shape)
    dev = _device_index(ring)
    with torch.cuda.device(dev):
        _lib.check(_lib.load().gsss_target_marginals(ring.data_ptr(), rows, first_row, n_rows, n_hist, n, d, m, dirs.data_ptr(),
                                                     int(dirs.shape[1]), bins, _lib.MARGINALS_STEP if steps else 0,
                                                     counts.data_ptr(), dev, current_stream_ptr(dev)))


def marginal_quantile(counts, edges, q):
    """Quantiles of histograms: counts (..., B) over the B equal bins between edges (B + 1,), q one level or several in [0, 1] ->
    (...,) or (..., Q).  With N the sum of a row, cum its running count and width = (edges[B] - edges[0]) / B: b is the first
    bin with cum_b >= q N (the first non-empty one for q = 0) and the value edges[b] + width (q N - cum_{b-1}) / count_b -- the
    draws of a bin taken as spread evenly over it.  NaN for an empty row.  CPU or CUDA tensors."""
    c = _t(counts).to(torch.float64)
    e = _t(edges).to(c)
    B = int(c.shape[-1])
    if c.ndim < 1 or B < 1 or tuple(e.shape) != (B + 1,):
        raise ValueError("counts must be (..., B) and edges (B + 1,)")
    qs = torch.as_tensor(q, dtype=torch.float64, device=c.device)
    if bool(((qs < 0) | (qs > 1)).any()):
        raise ValueError("a quantile level lies in [0, 1]")
    cum = torch.cumsum(c, -1)
    total = cum[..., -1:]
    want = total * qs.reshape(-1)                                                         # (..., Q)
    first = torch.searchsorted(cum, torch.full_like(total, 0.5))                          # the first non-empty bin
    b = torch.clamp(torch.maximum(torch.searchsorted(cum, want), first), max=B - 1)
    before = torch.where(b > 0, torch.gather(cum, -1, torch.clamp(b - 1, min=0)), torch.zeros_like(want))
    value = e[b] + (e[-1] - e[0]) / B * (want - before) / torch.gather(c, -1, b)
    value = torch.where(total > 0, value, torch.full_like(value, float("nan")))
    return value[..., 0] if qs.ndim == 0 else value


def from_target_marginals(counts, n_dirs, *, steps=False):
    """Per-target marginal densities and quantiles from the counts of `target_marginals` / `Sampler.summarize(marginals=)`:
    counts (M, S, B), S = P + (1 if steps else 0), P = n_dirs.  With N the sum of a row and w the bin width:

        marginal_edges (B + 1,) = linspace(-1, 1),  step_edges (B + 1,) = linspace(0, pi),
        marginal_density (M, P, B) = counts / (N w): it integrates to 1 over [-1, 1]; NaN where the row is empty,
        marginal_cdf (M, P, B) = running count / N, the value at every bin's upper edge,
        marginal_quantiles (M, P, 5) at q = 0.025, 0.25, 0.5, 0.75, 0.975 and marginal_median (M, P) = the one at 0.5,

    and with steps step_density (M, B) and step_quantiles (M, 5) of the geodesic step.  The quantile rule (`marginal_quantile`,
    which takes any q): with cum the running count, b is the first bin with cum_b >= q N, the value
    edge_b + w (q N - cum_{b-1}) / count_b.  CPU or CUDA tensors."""
    c = _t(counts)
    P, S = int(n_dirs), int(n_dirs) + (1 if steps else 0)
    if c.ndim != 3 or P < 0 or c.shape[1] != S or c.shape[2] < 2:
        raise ValueError(f"counts must be (M, {S}, B) for {P} directions{' and the steps' if steps else ''} (got {tuple(c.shape)})")
    B = int(c.shape[2])
    c = c.to(torch.float64)
    edges = torch.from_numpy(np.linspace(-1.0, 1.0, B + 1)).to(c.device)
    step_edges = torch.from_numpy(np.linspace(0.0, np.pi, B + 1)).to(c.device)
    qs = list(MARGINAL_QUANTILES)

    def density(rows, lo, hi):
        return rows / (rows.sum(-1, keepdim=True) * ((hi - lo) / B))
    u = c[:, :P]
    quantiles = marginal_quantile(u, edges, qs)
    out = {"marginal_edges": edges, "step_edges": step_edges, "marginal_density": density(u, -1.0, 1.0),
           "marginal_cdf": torch.cumsum(u, -1) / u.sum(-1, keepdim=True), "marginal_quantiles": quantiles,
           "marginal_median": quantiles[..., qs.index(0.5)]}
    if steps:
        out["step_density"] = density(c[:, P], 0.0, float(np.pi))
        out["step_quantiles"] = marginal_quantile(c[:, P], step_edges, qs)
    return out


LADDER_SLOTS = 10  # doubles per pair-chain of gsss_batch_ladder


def _ladder_fold(handle, lib, x, n_rows, n, target0, ladder, scratch, acc):
    """gsss_batch_ladder on the first n_rows rows of the contiguous block x (.., d, n) of the batch handle's members from
    target0 on; scratch holds 3 n_rows n doubles."""
    dev = _device_index(x)
    with torch.cuda.device(dev):
        _lib.check(lib.gsss_batch_ladder(handle, x.data_ptr(), n_rows, n, target0, ladder, scratch.data_ptr(), acc.data_ptr(),
                                         current_stream_ptr(dev)))


def target_ladder(batch, x, ladder, *, chain_major=False, acc=None):
    """The sums behind the log normalising constants along ladders of a TargetBatch's members, from draws you hold, on the
    device and without atomics (gsss_batch_ladder, include/gsss.h).

    x: a CUDA float64 tensor, component-major (rows, d, N) -- what `advance(..., thin=t)` returns -- or, with chain_major=True,
    (N, rows, d) -- what `sample(..., as_tensor=True)` returns.  The N chains cover all the batch's members, m = N / len(batch)
    each; the members form G = len(batch) / ladder ladders of R = `ladder` consecutive members, rung r colder than rung r + 1
    (`TargetBatch.tempered`'s order).  For every pair (a, b = a + 1) of neighbouring rungs and every chain i, each row gives
    u = l_a(x_b) - l_b(x_b) from the hotter member's draw and v = l_b(x_a) - l_a(x_a) from the colder member's, l_t the
    members' own `log_prob`, bit for bit; a row is used iff all four values are finite.  Returns, or continues, `acc`
    (G, R - 1, m, 10): draws used; M_u = max u and S_u = sum exp(u - M_u); sum u, sum u^2; M_v, S_v; sum v, sum v^2; draws
    skipped.  The result depends on the rows and their order alone: any cut into calls gives the same bits.  x is passed in
    blocks of rows, so that the scratch (three values per draw) never exceeds the size of x itself.
    -> `from_target_ladder`."""
    if not isinstance(x, torch.Tensor) or not x.is_cuda or x.dtype != torch.float64 or x.ndim != 3:
        raise ValueError("x must be a CUDA float64 tensor (rows, d, N), or (N, rows, d) with chain_major=True")
    N, rows, d = (int(v) for v in (x.shape if chain_major else (x.shape[2], x.shape[0], x.shape[1])))
    M, R = len(batch), int(ladder)
    if d != batch.d:
        raise ValueError(f"the batch's targets live in d={batch.d} (got {d})")
    if R < 2 or M % R:
        raise ValueError(f"the {M} targets of the batch are no run of whole ladders of {R} members (ladder >= 2)")
    if N < M or N % M:
        raise ValueError(f"the number of chains ({N}) must be a multiple of the batch's {M} targets, with at least one chain each")
    m = N // M
    acc = _accumulator("acc", acc, (M // R, R - 1, m, LADDER_SLOTS), x)
    if rows == 0:
        return acc
    tgt = batch._device_target(x.device, chains_per_target=m)
    xc = x.permute(1, 2, 0).contiguous() if chain_major else x.contiguous()
    per = max(1, min(rows, rows * d // 3))           # 3 per N doubles of scratch <= rows d N
    scratch = torch.empty(int(tgt.lib.gsss_ladder_scratch_doubles(per, N)), dtype=torch.float64, device=x.device)
    for r0 in range(0, rows, per):
        w = min(per, rows - r0)
        _ladder_fold(tgt.handle, tgt.lib, xc[r0:r0 + w], w, N, 0, R, scratch, acc)
    return acc


def from_target_ladder(acc, *, hot_log_z=None):
    """Log normalising constants from the accumulators of `target_ladder` / `Sampler.summarize(log_z=)`: acc (G, R - 1, m, 10),
    pair k of ladder g being the rungs (k, k + 1), rung 0 the coldest.  The per-chain sums are folded over the m chains with
    logsumexp and sums, where acc lives.  With n = the draws used over the pair's chains, every entry (G, R - 1):

        log_z_ratio_forward  = log( sum_i S_u e^{M_u} / n )      the stepping-stone (free-energy perturbation) estimate of
                               log Z_a / Z_b from the HOTTER member's draws, E_b[p_a / p_b];
        log_z_ratio_backward = -log( sum_i S_v e^{M_v} / n )     the same ratio from the colder member's draws, E_a[p_b / p_a];
        log_z_ratio          = log_z_ratio_forward.

    The forward estimate is the one reported and summed, the backward one a consistency check that is NOT averaged in: the
    hotter member's draws cover the colder member's mass, so the forward weights are tame, while the colder member's draws
    rarely reach where the hotter one has its mass and the backward weights are heavy-tailed at the cold end (a Watson target,
    kappa = 20, d = 5, beta halving, by quadrature: coefficient of variation of a weight 0.3 .. 1.0 forward, up to 5.1
    backward).

        log_z_lower = mean u,  log_z_upper = -mean v             the Jensen (Gibbs-Bogoliubov) bounds: for the very sample
                               log_z_lower <= log_z_ratio_forward and log_z_ratio_backward <= log_z_upper hold exactly;
        log_z_ratio_se       = the standard deviation of the m per-chain forward estimates / sqrt(m): a between-chain standard
                               error, itself known to a relative sqrt(2 / (m - 1)) (NaN for m = 1);
        used, skipped        = draws used and skipped, over the pair's chains;
        log_z (G, R)         = the sum of log_z_ratio from the hottest rung down, the hottest rung being 0, or hot_log_z (a
                               number or (G,): `TargetBatch.hot_log_z`) where given: log Z of every rung.  A ladder whose
                               hot_log_z is NaN (its hottest rung is not flat) keeps 0 there: its log_z is log Z relative to
                               its hottest rung, and differences between rungs are what they are either way.

    CPU or CUDA tensors."""
    acc = _t(acc).to(torch.float64)
    if acc.ndim != 4 or acc.shape[-1] != LADDER_SLOTS:
        raise ValueError("acc must be (G, R - 1, m, 10)")
    G, m = int(acc.shape[0]), int(acc.shape[2])
    n_i = acc[..., 0]
    used, skipped = n_i.sum(-1), acc[..., 9].sum(-1)
    neg_inf = torch.full_like(n_i, float("-inf"))
    lse_u = torch.where(n_i > 0, acc[..., 1] + torch.log(acc[..., 2]), neg_inf)   # per chain: log sum exp(u)
    lse_v = torch.where(n_i > 0, acc[..., 5] + torch.log(acc[..., 6]), neg_inf)
    forward = torch.logsumexp(lse_u, dim=-1) - torch.log(used)
    backward = -(torch.logsumexp(lse_v, dim=-1) - torch.log(used))
    per_chain = lse_u - torch.log(n_i)
    se = per_chain.std(dim=-1, unbiased=True) / float(np.sqrt(m)) if m > 1 else torch.full_like(forward, float("nan"))
    hot = torch.zeros(G, dtype=torch.float64, device=acc.device)
    if hot_log_z is not None:
        given = torch.as_tensor(hot_log_z, dtype=torch.float64).to(acc.device).reshape(-1)
        hot = hot + torch.where(torch.isnan(given), torch.zeros_like(given), given)
    down = torch.flip(torch.cumsum(torch.flip(forward, dims=[1]), dim=1), dims=[1])      # rung r: the pairs r .. R - 2
    log_z = torch.cat([down, torch.zeros((G, 1), dtype=torch.float64, device=acc.device)], dim=1) + hot[:, None]
    return {"log_z_ratio_forward": forward, "log_z_ratio_backward": backward, "log_z_ratio": forward,
            "log_z_lower": acc[..., 3].sum(-1) / used, "log_z_upper": -acc[..., 7].sum(-1) / used, "log_z_ratio_se": se,
            "used": used, "skipped": skipped, "log_z": log_z}


def ring_plan(rest, window, hist_rows, seen):
    """How `Sampler.summarize` lays 1 + rest retained draws into its one reused buffer, in integers alone: windows of up to
    `window` rows behind H = hist_rows rows of history, `seen` (<= H) of which an earlier call left.  -> (rows, draw0, windows, keep):
    rows = H + window, the buffer's; draw0 = (row, 1, n_hist) of draw 0, or None where H = 0 and the state itself is folded as a
    window of one; windows = [(first_row, n_rows, n_hist), ..] of the draws after it; keep: the rows that hold the last
    min(H, draws so far) draws at the end, oldest first -- the next call's history.  Without history every window starts at row 0.
    With it the buffer is a ring: the earlier call's rows lie at 0 .. seen - 1, draw 0 at row `seen`, the windows follow one behind
    the other, each cut at the ring's end so that none wraps; the n_hist = min(H, draws so far) rows before a window, taken round
    the ring's end, are the draws before it."""
    H, rows = hist_rows, hist_rows + window
    if not H:
        return rows, None, [(0, min(window, rest - done), 0) for done in range(0, rest, window)], []
    draw0, windows = (seen, 1, seen), []
    pos, seen, done = seen + 1, seen + 1, 0
    while done < rest:
        pos %= rows
        w = min(window, rest - done, rows - pos)
        windows.append((pos, w, min(H, seen)))
        pos, seen, done = pos + w, seen + w, done + w
    return rows, draw0, windows, [(pos - min(H, seen) + i) % rows for i in range(min(H, seen))]


class TargetMoments:
    """What `Sampler.summarize` returns: the per-target accumulators of a run (`acc` (M, rows), `chain_sum` (d, n), device
    tensors; see `target_moments`) and what they belong to.  stats() -> `from_target_moments`.  Everything a statistic of
    `summarize` needs is here: `begin` allocates what it keeps, `check_continues` says why into= cannot take it up, `fold` adds one
    window to it, `stats` reports it.

    With `summarize(lags=L)` also the lagged products of every coordinate: `lags` = L, `acov` (M, d, L + 1, 3) (see
    `target_autocov`) and `hist`, the last min(L, draws) retained rows (h, d, n), from which into= goes on; with log_prob=True
    `lp_acov` (M, 1, L + 1, 3) and `lp_hist` (h, 1, n) for the log-density series.  stats() then adds acf, iat, ess_within,
    iat_truncated (`from_target_autocov`) and lp_acf, lp_iat, lp_ess_within, lp_iat_truncated.

    With `summarize(log_prob=True)` also the log-density trace: `lp_acc` (M, 3) -- count, sum, sum of squares of log_prob over
    the target's draws --, `lp_chain_sum` (n,), and the best draw seen per target, `lp_best` (M,) and `x_best` (M, d): the maximum
    of log_prob over all retained draws (ties: the earliest draw, then the lowest chain).  stats() then adds lp_mean, lp_var,
    lp_rhat, lp_ess_between (`from_scalar_moments`), lp_best and x_best.

    With `summarize(mixing=)` also the step, hop and mode counts of every target against its own directions: `mix_step` (M, 2)
    and `mix_counts` (M, 3 + K [+ K K]) (see `target_mixing`), `mix_modes` = K, `mix_weights` (M, K) or None, the directions
    `mix_dirs` (M, 1 + K, d) and whether the transitions are counted, from which into= goes on; without lags `hist` is the one
    last retained row, so that the pair at the seam of two calls counts exactly once.  stats() then adds geodesic_step,
    geodesic_step_sd, hop_frequency, mode_occupancy and, where they apply, mode_transitions, mode_switch_frequency and mode_kl
    (`from_target_mixing`).

    With `summarize(log_z=)` also the sums behind the log normalising constants along the ladders of the sampler's members:
    `ladder` = R, `ladder_acc` (G, R - 1, m, 10) (see `target_ladder`), from which into= goes on, and `ladder_hot_log_z` (G,), the
    batch's `hot_log_z` (NaN where the hottest rung is not flat).  stats() then adds log_z_ratio (the forward estimate; the
    backward one is reported beside it as a check, not averaged in), log_z_ratio_forward, log_z_ratio_backward, log_z_lower,
    log_z_upper, log_z_ratio_se, used, skipped, log_z and hot_log_z (`from_target_ladder`).

    With `summarize(marginals=)` also the marginal histograms of every target along its own directions: `marg_counts` (M, S, B)
    int64 (see `target_marginals`), the directions `marg_dirs` (M, P, d), `marg_bins` = B and `marg_steps`, whether series P
    counts the geodesic steps, from which into= goes on; with the steps and without lags `hist` is the one last retained row, so
    that the pair at the seam of two calls counts exactly once.  stats() then adds marginal_edges, step_edges, marginal_density,
    marginal_cdf, marginal_quantiles, marginal_median and, with the steps, step_density and step_quantiles
    (`from_target_marginals`); `quantile(q)` gives the marginals' quantiles at any level."""

    def __init__(self, acc, chain_sum, d, chains_per_target, second_moment, lp_acc=None, lp_chain_sum=None, lp_best=None,
                 x_best=None):
        self.acc, self.chain_sum, self.d = acc, chain_sum, int(d)
        self.chains_per_target, self.second_moment = int(chains_per_target), bool(second_moment)
        self.lp_acc, self.lp_chain_sum, self.lp_best, self.x_best = lp_acc, lp_chain_sum, lp_best, x_best
        self.lags, self.acov, self.hist, self.lp_acov, self.lp_hist = None, None, None, None, None
        self.mix_step, self.mix_counts, self.mix_modes, self.mix_weights = None, None, None, None
        self.mix_dirs, self.mix_transitions = None, False
        self.ladder, self.ladder_acc, self._ladder_hot, self._ladder_source = None, None, None, None
        self.marg_counts, self.marg_dirs, self.marg_bins, self.marg_steps = None, None, None, False

    @classmethod
    def begin(cls, n, d, chains_per_target, device, *, second_moment=None, log_prob=False, lags=None, mixing=None, ladder=None,
              ladder_source=None, marginals=None):
        """Zeroed accumulators of n chains in d dimensions on `device` and of the features asked for: log_prob, lags = L, mixing =
        dict(hop, modes, weights, transitions), ladder = R with ladder_source = (batch, first ladder) for `ladder_hot_log_z`,
        marginals = dict(bins, directions, steps)."""
        m = int(chains_per_target)
        M = n // m
        full, rows = _moments_form(d, second_moment)

        def zeros(*shape, dtype=torch.float64):
            return torch.zeros(shape, dtype=dtype, device=device)
        tm = cls(zeros(M, rows), zeros(d, n), d, m, full)
        if log_prob:
            tm.lp_acc, tm.lp_chain_sum, tm.x_best = zeros(M, 3), zeros(n), zeros(M, d)
            tm.lp_best = torch.full((M,), float("-inf"), dtype=torch.float64, device=device)
        if lags is not None:
            tm.lags = int(lags)
            tm.acov = zeros(M, d, tm.lags + 1, 3)
            if log_prob:
                tm.lp_acov = zeros(M, 1, tm.lags + 1, 3)
        if mixing is not None:
            tm.mix_dirs, tm.mix_modes = _mixing_dirs(mixing["hop"], mixing["modes"], M, d, device)
            tm.mix_transitions = mixing["transitions"]
            if mixing["weights"] is not None:
                w = _t(mixing["weights"]).to(torch.float64)
                w = w[None].expand(M, -1) if w.ndim == 1 else w
                if tm.mix_modes == 0 or tuple(w.shape) != (M, tm.mix_modes):
                    raise ValueError(f"weights must be (K,) or (M, K) = ({M}, {tm.mix_modes}), one per mode direction")
                tm.mix_weights = w.contiguous().to(device)
            tm.mix_step = zeros(M, 2)
            tm.mix_counts = zeros(M, 3 + tm.mix_modes + (tm.mix_modes ** 2 if tm.mix_transitions else 0), dtype=torch.int64)
        if ladder is not None:
            tm.ladder, tm._ladder_source = ladder, ladder_source
            tm.ladder_acc = zeros(M // ladder, ladder - 1, m, LADDER_SLOTS)
        if marginals is not None:
            tm.marg_dirs, P = _marginal_dirs(marginals["directions"], M, d, device)
            tm.marg_steps = bool(marginals["steps"])
            tm.marg_bins = _marginal_shape(marginals["bins"], P, tm.marg_steps)
            tm.marg_counts = zeros(M, P + (1 if tm.marg_steps else 0), tm.marg_bins, dtype=torch.int64)
        return tm

    def check_continues(self, n, d, chains_per_target, *, second_moment=None, log_prob=False, lags=None, mixing=None, ladder=None,
                        marginals=None):
        """ValueError unless into= can go on with this call: the same chains and form, and no feature it was begun without."""
        full, rows = _moments_form(d, self.second_moment if second_moment is None else second_moment)
        M = n // chains_per_target
        if (self.d != d or self.chains_per_target != chains_per_target or self.second_moment != full
                or tuple(self.acc.shape) != (M, rows) or tuple(self.chain_sum.shape) != (d, n)):
            raise ValueError("into= continues a summary of the same chains, chains_per_target and second-moment form")
        if log_prob and self.lp_acc is None:
            raise ValueError("into= was begun without log_prob: its draws so far were not evaluated, so it cannot take log_prob up")
        if lags is not None and self.lags != int(lags):
            raise ValueError("into= was begun without these lags: the lagged products of its draws so far were not kept, so it "
                             "cannot take them up")
        if mixing is not None and self.mix_step is None:
            raise ValueError("into= was begun without mixing: the steps and counts of its draws so far were not kept, so it "
                             "cannot take them up")
        if ladder is not None and self.ladder != ladder:
            raise ValueError("into= was begun without log_z along these ladders: the ratios of its draws so far were not kept, so "
                             "it cannot take them up")
        if marginals is not None and (self.marg_counts is None or self.marg_bins != int(marginals["bins"])
                                      or int(self.marg_dirs.shape[1]) != _n_marginal_dirs(marginals["directions"], d)
                                      or self.marg_steps != bool(marginals["steps"])):
            raise ValueError("into= was begun without these marginals (bins, number of directions, steps): the histograms of its "
                             "draws so far were not kept, so it cannot take them up")

    @property
    def n_targets(self):
        return int(self.acc.shape[0])

    @property
    def hist_rows(self):
        """Rows of history the ring of `summarize` keeps before a window: the lags, one at least for the pair of a step."""
        return max(self.lags or 0, 1) if self.mix_step is not None or self.marg_steps else self.lags or 0

    @property
    def hist_seen(self):
        return 0 if self.hist is None else int(self.hist.shape[0])

    def load_hist(self, ring, lp_ring):
        """The rows an earlier call kept become the ring's first."""
        if self.hist_seen:
            ring[:self.hist_seen] = self.hist
            if self.lp_acc is not None:
                lp_ring[:self.hist_seen] = self.lp_hist[:, 0]

    def store_hist(self, ring, lp_ring, rows):
        """Keep these rows of the ring, oldest first, for the call that continues the summary."""
        last = torch.tensor(rows, device=ring.device)
        self.hist = ring[last]
        if self.lp_acc is not None:
            self.lp_hist = lp_ring[last][:, None, :]

    def fold(self, ring, lp_ring, first, n_rows, n_hist, batch=None, scratch=None):
        """Fold rows first .. first + n_rows of the contiguous ring (rows, d, n), behind the n_hist rows before them round the
        ring's end, into every accumulator kept.  lp_ring (rows, n) receives their log-densities; batch = (library, handle, first
        target) of the TargetBatch they are evaluated under; scratch: gsss_ladder_scratch_doubles(n_rows, n) doubles."""
        x, m, L, n = ring[first:first + n_rows], self.chains_per_target, self.lags or 0, int(ring.shape[2])
        target_moments(x, m, second_moment=self.second_moment, acc=self.acc, chain_sum=self.chain_sum)
        if self.lp_acc is not None:
            lib, handle, target0 = batch
            lp, x, dev = lp_ring[first:first + n_rows], x.contiguous(), _device_index(ring)
            with torch.cuda.device(dev):
                _lib.check(lib.gsss_batch_logprob_draws(handle, x.data_ptr(), n_rows, n, target0, lp.data_ptr(),
                                                        current_stream_ptr(dev)))
            scalar_moments(lp, m, acc=self.lp_acc, chain_sum=self.lp_chain_sum)
            self.update_best(lp, x)
        if L:
            _autocov_fold(ring, first, n_rows, min(L, n_hist), m, L, self.acov)
            if self.lp_acov is not None:
                _autocov_fold(lp_ring[:, None, :], first, n_rows, min(L, n_hist), m, L, self.lp_acov)
        if self.mix_step is not None:
            _mixing_fold(ring, first, n_rows, min(1, n_hist), m, self.mix_dirs, self.mix_modes, self.mix_transitions, self.mix_step,
                         self.mix_counts)
        if self.marg_counts is not None:
            _marginals_fold(ring, first, n_rows, min(1, n_hist), m, self.marg_dirs, self.marg_bins, self.marg_steps, self.marg_counts)
        if self.ladder is not None:
            lib, handle, target0 = batch
            _ladder_fold(handle, lib, x.contiguous(), n_rows, n, target0, self.ladder, scratch, self.ladder_acc)

    @property
    def ladder_hot_log_z(self):
        """(G,) numpy: `TargetBatch.hot_log_z` of the ladders summarised, taken from the batch when first asked for."""
        if self._ladder_hot is None and self._ladder_source is not None:
            batch, g0 = self._ladder_source
            self._ladder_hot = batch.hot_log_z(self.ladder)[g0:g0 + int(self.ladder_acc.shape[0])]
        return self._ladder_hot

    def update_best(self, values, x):
        """Fold a window into the running best draw: values (w, n) the log_prob of the draws x (w, d, n).  A later draw replaces
        the best only if it is strictly better."""
        best, row, chain = best_draw(values, self.chains_per_target)
        better = best > self.lp_best
        self.lp_best = torch.where(better, best, self.lp_best)
        self.x_best = torch.where(better[:, None], x[row, :, chain], self.x_best)

    def stats(self):
        out = from_target_moments(self.acc, self.d, chain_sum=self.chain_sum, chains_per_target=self.chains_per_target,
                                  second_moment=self.second_moment)
        if self.lp_acc is not None:
            lp = from_scalar_moments(self.lp_acc, self.lp_chain_sum, self.chains_per_target)
            out.update(lp_mean=lp["mean"], lp_var=lp["var"], lp_rhat=lp["rhat"], lp_ess_between=lp["ess_between"])
        if self.lp_best is not None:
            out.update(lp_best=self.lp_best, x_best=self.x_best)
        if self.acov is not None:
            per_chain = self.acc[:, 0] / self.chains_per_target
            out.update(from_target_autocov(self.acov, self.chains_per_target, per_chain))
            if self.lp_acov is not None:
                lp = from_target_autocov(self.lp_acov, self.chains_per_target, per_chain)
                out.update({"lp_" + key: val[:, 0] for key, val in lp.items()})
        if self.mix_step is not None:
            out.update(from_target_mixing(self.mix_step, self.mix_counts, self.mix_modes, weights=self.mix_weights))
        if self.ladder_acc is not None:
            out.update(from_target_ladder(self.ladder_acc, hot_log_z=self.ladder_hot_log_z))
            out["hot_log_z"] = torch.as_tensor(self.ladder_hot_log_z, dtype=torch.float64).to(self.ladder_acc.device)
        if self.marg_counts is not None:
            out.update(from_target_marginals(self.marg_counts, int(self.marg_dirs.shape[1]), steps=self.marg_steps))
        return out

    def quantile(self, q):
        """The quantiles of every target's marginals at the level(s) q in [0, 1]: (M, P) or (M, P, Q) (`marginal_quantile`)."""
        if self.marg_counts is None:
            raise ValueError("this summary was begun without marginals: summarize(marginals=...) keeps the histograms")
        P = int(self.marg_dirs.shape[1])
        edges = torch.from_numpy(np.linspace(-1.0, 1.0, self.marg_bins + 1)).to(self.marg_counts.device)
        return marginal_quantile(self.marg_counts[:, :P], edges, q)


def _average_ranks(flat):
    """scipy.stats.rankdata(method='average') of a 1-D tensor: 1-based ranks, ties share the mean of their ranks."""
    order = torch.argsort(flat, stable=True)
    sorted_vals = flat[order]
    n = flat.numel()
    pos = torch.arange(1, n + 1, dtype=torch.float64, device=flat.device)
    # runs of equal values: every member gets the mean position of the run
    _, inverse, counts = torch.unique_consecutive(sorted_vals, return_inverse=True, return_counts=True)
    ends = torch.cumsum(counts, 0).to(torch.float64)
    mean_pos = ends - (counts.to(torch.float64) - 1.0) / 2.0
    ranks = torch.empty(n, dtype=torch.float64, device=flat.device)
    ranks[order] = mean_pos[inverse]
    del pos
    return ranks


def _autocov_fft(z):
    """Biased autocovariance of every row (divided by n), lags 0 .. n-1, by the convolution theorem on a zero-padded transform."""
    n = z.shape[-1]
    m = 1 << int(2 * n - 1).bit_length()
    c = z - z.mean(-1, keepdim=True)
    f = torch.fft.rfft(c, n=m, dim=-1)
    return torch.fft.irfft(f * f.conj(), n=m, dim=-1)[..., :n] / n


def ess_bulk(x, relative=False):
    """Rank-normalised split-chain bulk effective sample size of a scalar quantity over several chains, x (chains, draws) --
    what `arviz.ess(..., method="bulk")` computes and the reference's experiments report as "relative ESS"
    (scripts/bingham.py:43-57: the draws projected on the target's mode, 10 chains, az.ess(relative=True);
    scripts/vMF_diagnostics.py:466-478).  Restated from the published algorithm (Vehtari, Gelman, Simpson, Carpenter, Buerkner
    2021, "Rank-normalization, folding, and localization: an improved R-hat", section 3, as implemented in Stan and ArviZ 0.x;
    arviz itself is not installed in this image):
      1. split every chain into its two halves (2 C chains of N = draws // 2);
      2. replace the pooled values by their average ranks r, z = Phi^-1((r - 3/8) / (S + 1/4)), S = 2 C N;
      3. per-chain biased autocovariances (FFT), W = mean_c acov_c[0] N / (N - 1), var+ = W (N - 1) / N + var_c(chain means);
      4. rho_t = 1 - (W - mean_c acov_c[t]) / var+, Geyer's initial positive sequence over pairs (rho_2k + rho_2k+1 > 0), then the
         initial monotone sequence;
      5. tau = -1 + 2 sum_{t <= max_t} rho_t + rho_{max_t + 1}, floored at 1 / log10(S); ESS = S / tau (relative: 1 / tau).
    The ranking, the transforms and the correlations run where `x` lives (a CUDA tensor stays on the device; 10 chains x 10^5
    draws take milliseconds); the sequential truncation runs on the host over the S / (2 C) lags."""
    t = _t(x).to(torch.float64)
    if t.dim() != 2 or t.shape[1] < 4:
        raise ValueError("ess_bulk takes (chains, draws) with at least 4 draws")
    half = t.shape[1] // 2
    split = torch.cat([t[:, :half], t[:, t.shape[1] - half:]], dim=0)            # (2 C, N)
    n_chain, n_draw = split.shape
    size = split.numel()
    if float(split.max() - split.min()) < 1e-15:
        return float(1.0 if relative else size)
    ranks = _average_ranks(split.reshape(-1))
    z = torch.special.ndtri((ranks - 0.375) / (size + 0.25)).reshape(n_chain, n_draw)
    acov = _autocov_fft(z)                                                      # (2 C, N)
    mean_acov = acov.mean(0)
    mean_var = float(mean_acov[0]) * n_draw / (n_draw - 1.0)
    var_plus = mean_var * (n_draw - 1.0) / n_draw
    if n_chain > 1:
        var_plus += float(z.mean(1).var(unbiased=True))
    rho = (1.0 - (mean_var - mean_acov) / var_plus).cpu().numpy()               # rho_hat for every lag
    rho_t = np.zeros(n_draw)
    rho_even, rho_odd = 1.0, float(rho[1])
    rho_t[0], rho_t[1] = rho_even, rho_odd
    k = 1
    while k < n_draw - 3 and rho_even + rho_odd > 0.0:                          # Geyer's initial positive sequence
        rho_even, rho_odd = float(rho[k + 1]), float(rho[k + 2])
        if rho_even + rho_odd >= 0.0:
            rho_t[k + 1], rho_t[k + 2] = rho_even, rho_odd
        k += 2
    max_t = k - 2
    if rho_even > 0.0:
        rho_t[max_t + 1] = rho_even
    k = 1
    while k <= max_t - 2:                                                       # Geyer's initial monotone sequence
        if rho_t[k + 1] + rho_t[k + 2] > rho_t[k - 1] + rho_t[k]:
            rho_t[k + 1] = (rho_t[k - 1] + rho_t[k]) / 2.0
            rho_t[k + 2] = rho_t[k + 1]
        k += 2
    tau = -1.0 + 2.0 * float(np.sum(rho_t[: max_t + 1])) + float(np.sum(rho_t[max_t + 1: max_t + 2]))
    tau = max(tau, 1.0 / np.log10(size))
    return float((1.0 if relative else size) / tau)
