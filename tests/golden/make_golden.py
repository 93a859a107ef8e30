"""Generate the golden fixtures in this directory from the REFERENCE's own code.

Run in the build container only (needs /root/reference; the GPU box never runs
this):   python tests/golden/make_golden.py

It imports the reference modules SOBER/_settings.py, _utils.py, _weights.py,
_rchq.py (no stubs) and _gp.py, _kernel.py (import-time stubs for gpytorch /
botorch, which are not installed) under a dummy ``SOBER`` package, feeds them
seeded inputs through a duck-typed GP model, and stores inputs + outputs +
per-level traces as ``.npz``.  gpytorch is absent, so the model's
``covar_module.forward`` is the oracle's restated base kernel
(oracle/sober_oracle.py:base_kernel) -- that boundary is parity-unpinned; all
code above it (predictive_covariance, Kernel, recombination, CAR, make_cov_psd,
KMeans, cleansing_weights, batch_tanimoto_sim) is the reference's own.

Nothing from /root/reference is copied: fixtures are data (inputs, outputs).
"""
import contextlib
import importlib.util
import os
import sys
import types
import warnings

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
REF = "/root/reference/SOBER"

from oracle import sober_oracle as O  # noqa: E402
from tests.golden.synth import synth, build_spec, checksum, calc_obj_fn, load_case, SEED_CALL  # noqa: E402


# --------------------------------------------------------------------------- #
# reference loader
# --------------------------------------------------------------------------- #
def _install_stubs():
    def mod(name):
        m = types.ModuleType(name)
        sys.modules[name] = m
        return m
    g = mod("gpytorch")
    for sub in ("models", "means", "likelihoods", "constraints", "mlls", "distributions",
                "settings", "priors", "kernels"):
        setattr(g, sub, mod("gpytorch." + sub))
    g.models.ExactGP = object
    g.means.ZeroMean = object
    g.likelihoods.GaussianLikelihood = object
    g.constraints.Interval = object
    g.mlls.ExactMarginalLogLikelihood = object
    g.distributions.MultivariateNormal = object
    tp = mod("gpytorch.priors.torch_priors")
    tp.GammaPrior = object
    g.priors.torch_priors = tp
    g.settings.fast_pred_var = contextlib.nullcontext
    g.settings.fast_computations = contextlib.nullcontext
    g.settings.cholesky_jitter = lambda **kw: contextlib.nullcontext()
    b = mod("botorch")
    b.fit = mod("botorch.fit")
    b.fit.fit_gpytorch_mll = lambda *a, **k: None


def load_reference():
    _install_stubs()
    pkg = types.ModuleType("SOBER")
    pkg.__path__ = [REF]
    sys.modules["SOBER"] = pkg
    out = {}
    for name in ("_settings", "_utils", "_weights", "_rchq", "_gp", "_kernel", "_pi"):
        spec = importlib.util.spec_from_file_location(f"SOBER.{name}", f"{REF}/{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"SOBER.{name}"] = m
        spec.loader.exec_module(m)
        out[name] = m
    out["_settings"].setting_parameters(device=torch.device("cpu"), dtype=torch.double)
    return out


class _Pred:
    def __init__(self, mean, variance):
        self.mean, self.variance = mean, variance
        self.loc = mean


class _Lik:
    def __init__(self, noise):
        self.noise = torch.tensor([noise], dtype=torch.double)

    def eval(self):
        return self

    def __call__(self, pred):
        return _Pred(pred.mean, pred.variance + self.noise)


class DuckModel:
    """The attributes the reference path touches: covar_module.forward,
    train_inputs, likelihood.noise, prediction_strategy.covar_cache, eval(), __call__."""

    def __init__(self, spec: O.GPSpec):
        self.spec = spec
        self.train_inputs = (spec.X_obs,)
        self.likelihood = _Lik(spec.noise)
        self.covar_module = types.SimpleNamespace(forward=lambda x, y: O.base_kernel(spec, x, y))
        self.prediction_strategy = types.SimpleNamespace(covar_cache=spec.S_cache)

    def eval(self):
        return self

    def __call__(self, x):
        mean, var = O.predict(x, self.spec)
        return _Pred(mean, var - self.spec.noise)            # latent variance; the likelihood adds the noise


CASES = [
    dict(name="cfg1_rbf_ard", kind=O.RBF, mode="predictive_covariance", N=2000, M=100, d=2, b=10,
         n_obs=30, ard=True, seed=0),
    dict(name="rbf_noleft", kind=O.RBF, mode="predictive_covariance", N=2560, M=64, d=3, b=10,
         n_obs=20, seed=1),
    dict(name="rbf_b30", kind=O.RBF, mode="predictive_covariance", N=3000, M=120, d=5, b=30,
         n_obs=50, seed=2, outputscale=1.7),
    dict(name="matern_b20", kind=O.MATERN52, mode="predictive_covariance", N=3000, M=100, d=6, b=20,
         n_obs=40, seed=3, ard=True),
    dict(name="tanimoto_weighted", kind=O.TANIMOTO, mode="weighted_predictive_covariance", N=1500,
         M=64, d=128, b=10, n_obs=25, seed=4, mean_const=0.3),
    dict(name="rbf_weighted", kind=O.RBF, mode="weighted_predictive_covariance", N=2000, M=80, d=4,
         b=10, n_obs=30, seed=5, mean_const=1.0),
    dict(name="rbf_zero_weights", kind=O.RBF, mode="predictive_covariance", N=2500, M=64, d=3, b=10,
         n_obs=20, seed=6, zero_frac=0.3),
    dict(name="rbf_basekernel", kind=O.RBF, mode="kernel", N=1200, M=50, d=3, b=8, n_obs=10, seed=7),
    dict(name="rbf_calc_obj", kind=O.RBF, mode="predictive_covariance", N=2000, M=64, d=3, b=10,
         n_obs=20, seed=8, calc_obj=True),
    dict(name="rbf_tiny_direct", kind=O.RBF, mode="predictive_covariance", N=18, M=12, d=2, b=10,
         n_obs=6, seed=9),      # n+1 < N <= 2b: straight to the final direct level
    dict(name="rbf_medium", kind=O.RBF, mode="predictive_covariance", N=20000, M=200, d=6, b=50,
         n_obs=100, seed=10, store_inputs=False),
    dict(name="matern_medium", kind=O.MATERN52, mode="predictive_covariance", N=12000, M=200, d=6,
         b=100, n_obs=100, seed=11, store_inputs=False),
    dict(name="cfg2_rbf", kind=O.RBF, mode="predictive_covariance", N=100000, M=500, d=10, b=100,
         n_obs=200, seed=0, store_inputs=False, slim=True),
]

def run_reference(ref, case, inp, threads=None):
    spec = build_spec(case, inp)
    model = DuckModel(spec)
    kernel = ref["_kernel"].Kernel(model, mode=case["mode"])
    rchq = ref["_rchq"]
    rec = dict(levels=[], U=None, gram_in=None, gram_out=None)

    orig_car, orig_sparsify = rchq.Tchernychova_Lyons_CAR, rchq.ker_svd_sparsify
    tm_cls = ref["_utils"].SafeTensorOperator
    orig_psd = tm_cls.make_cov_psd

    def car_wrap(X, mu, tm, DEBUG=False):
        Xc, muc = X.clone(), mu.clone()
        out = orig_car(X, mu, tm, DEBUG)
        rec["levels"].append(dict(X_tmp=Xc, tot_weights=muc, w_star=out[0].clone(),
                                  idx_star=out[1].clone()))
        return out

    def sparsify_wrap(pt, s, kernel, tm):
        S, U = orig_sparsify(pt, s, kernel, tm)
        rec["U"] = U.clone()
        return S, U

    def psd_wrap(self, cov):
        rec["gram_in"] = cov.clone()
        out = orig_psd(self, cov)
        rec["gram_out"] = out.clone()
        return out

    rchq.Tchernychova_Lyons_CAR = car_wrap
    rchq.ker_svd_sparsify = sparsify_wrap
    tm_cls.make_cov_psd = psd_wrap
    old_threads = torch.get_num_threads()
    if threads:
        torch.set_num_threads(threads)
    try:
        X_cand = torch.from_numpy(inp["X_cand"].copy())
        X_nys = torch.from_numpy(inp["X_nys"].copy())
        mu = torch.from_numpy(inp["mu0"].copy())
        torch.manual_seed(SEED_CALL)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            idx, w = rchq.recombination(
                X_cand, X_nys, case["b"], kernel, torch.device("cpu"), torch.double,
                init_weights=mu, calc_obj=calc_obj_fn if case.get("calc_obj") else None)
    finally:
        rchq.Tchernychova_Lyons_CAR = orig_car
        rchq.ker_svd_sparsify = orig_sparsify
        tm_cls.make_cov_psd = orig_psd
        torch.set_num_threads(old_threads)
    rec.update(idx=idx.clone(), w=w.clone(), mu_after=mu.clone(), spec=spec)
    return rec


def gen_recombination(ref):
    for case in CASES:
        inp = synth(case)
        rec = run_reference(ref, case, inp)
        rec1 = run_reference(ref, case, inp, threads=1)
        same_idx = bool(torch.equal(rec["idx"], rec1["idx"]))
        dw = float(((rec["w"] - rec1["w"]).abs() / rec["w"].abs()).max()) if same_idx else float("nan")
        spec = rec["spec"]
        W = spec.S_cache @ spec.S_cache.T
        condW = float(torch.linalg.cond(W))
        slim = case.get("slim", False)
        out = dict(
            kind=case["kind"], mode=case["mode"], b=case["b"], seed=case["seed"], seed_call=SEED_CALL,
            N=case["N"], M=case["M"], d=case["d"], n_obs=case["n_obs"],
            ard=case.get("ard", False), bit_p=case.get("bit_p", 0.1), zero_frac=case.get("zero_frac", 0.0),
            calc_obj=bool(case.get("calc_obj", False)),
            outputscale=spec.outputscale, noise=spec.noise, mean_const=spec.mean_const,
            lengthscale=spec.lengthscale.numpy(),
            idx=rec["idx"].numpy(), w=rec["w"].numpy(),
            mu_after_idx=torch.nonzero(rec["mu_after"]).flatten().numpy(),
            mu_after_val=rec["mu_after"][rec["mu_after"] != 0].numpy(),
            n_levels=len(rec["levels"]),
            self_threads_same_idx=same_idx, self_threads_dw=dw, condW=condW,
            cks_X_cand=checksum(inp["X_cand"]), cks_mu0=checksum(inp["mu0"]),
            cks_X_nys=checksum(inp["X_nys"]), cks_S_cache=checksum(spec.S_cache.numpy()),
        )
        if case.get("store_inputs", True):
            out.update(X_cand=inp["X_cand"], X_nys=inp["X_nys"], mu0=inp["mu0"], X_obs=inp["X_obs"],
                       y_obs=inp["y_obs"], S_cache=spec.S_cache.numpy(),
                       alpha=spec.alpha.numpy())
        if not slim:
            out.update(U=rec["U"].numpy(), gram_in=rec["gram_in"].numpy(),
                       gram_out=rec["gram_out"].numpy())
        else:
            out.update(cks_U=checksum(rec["U"].numpy()))
        for i, lv in enumerate(rec["levels"]):
            out[f"L{i}_tot_weights"] = lv["tot_weights"].numpy()
            out[f"L{i}_idx_star"] = lv["idx_star"].numpy()
            out[f"L{i}_w_star"] = lv["w_star"].numpy()
            if slim:
                out[f"L{i}_cks_X_tmp"] = checksum(lv["X_tmp"].numpy())
                out[f"L{i}_shape_X_tmp"] = np.array(lv["X_tmp"].shape)
            else:
                out[f"L{i}_X_tmp"] = lv["X_tmp"].numpy()
        path = os.path.join(HERE, f"recomb_{case['name']}.npz")
        np.savez_compressed(path, **out)
        print(f"{case['name']:22s} levels={len(rec['levels']):2d} |idx|={len(rec['idx']):3d} "
              f"threads1-vs-8: same_idx={same_idx} dw={dw:.2e} cond(W)={condW:.2e} "
              f"{os.path.getsize(path) / 1024:.0f} KB")


def gen_kmeans(ref):
    KMeans = ref["_weights"].KMeans
    rng = np.random.default_rng(100)
    out = {}
    x = rng.random((3000, 4))
    cl, c = KMeans(torch.from_numpy(x.copy()), K=50)
    out.update(a_x=x, a_K=50, a_cl=cl.numpy(), a_c=c.numpy())
    # duplicate rows in the first K -> an empty cluster -> NaN centroid
    x2 = rng.random((500, 3))
    x2[3] = x2[1]
    cl2, c2 = KMeans(torch.from_numpy(x2.copy()), K=8)
    out.update(b_x=x2, b_K=8, b_cl=cl2.numpy(), b_c=c2.numpy())
    x3 = rng.random((20000, 6))
    cl3, c3 = KMeans(torch.from_numpy(x3.copy()), K=200)
    out.update(c_seed=100, c_N=20000, c_d=6, c_K=200, c_cks_x=checksum(x3), c_c=c3.numpy(),
               c_cl=cl3.numpy().astype(np.int32))
    np.savez_compressed(os.path.join(HERE, "kmeans.npz"), **out)
    print("kmeans: NaN centroids in case b:", int(np.isnan(c2.numpy()).any(axis=1).sum()))


def gen_weights(ref):
    WS = ref["_weights"].WeightsStabiliser
    ws = WS()
    rng = np.random.default_rng(200)
    w = rng.random(1000)
    w[::7] = 1e-9
    w[5] = np.inf
    w[11] = np.nan
    w[13] = -1.0
    out = dict(eps=ws.eps_weights, a_in=w.copy())
    out["a_out"] = ws.cleansing_weights(torch.from_numpy(w.copy())).numpy()
    z = np.zeros(16)
    out["b_in"] = z.copy()
    out["b_out"] = ws.cleansing_weights(torch.from_numpy(z.copy())).numpy()
    w3 = rng.random(500) + 0.01
    torch.manual_seed(7)
    out["c_in"] = w3.copy()
    out["c_idx_deweighted"] = ws.deweighted_resampling(torch.from_numpy(w3.copy()), 40).numpy()
    torch.manual_seed(8)
    out["c_idx_weighted"] = ws.weighted_resampling(torch.from_numpy(w3 / w3.sum()), 40).numpy()
    out["check_true"] = ws.check_weights(torch.from_numpy(w3))
    out["check_false"] = ws.check_weights(torch.from_numpy(np.r_[np.ones(10), np.zeros(5)]))
    np.savez_compressed(os.path.join(HERE, "weights.npz"), **out)


def gen_psd(ref):
    tm = ref["_utils"].SafeTensorOperator()
    rng = np.random.default_rng(300)
    out = {}
    A = rng.standard_normal((40, 40))
    spd = A @ A.T + 40 * np.eye(40)
    spd = 0.5 * (spd + spd.T)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        out["a_in"] = spd
        out["a_out"] = tm.make_cov_psd(torch.from_numpy(spd.copy())).numpy()
        t = np.linspace(0, 1, 40)               # numerically singular RBF Gram with entries > 0:
        low = np.exp(-0.5 * (t[:, None] - t[None, :]) ** 2 / 0.5 ** 2)   # Cholesky fails -> jitter ladder
        out["b_in"] = low
        out["b_out"] = tm.make_cov_psd(torch.from_numpy(low.copy())).numpy()
        ns = spd + 1e-13 * rng.standard_normal((40, 40))   # PD but not exactly symmetric
        out["c_in"] = ns
        out["c_out"] = tm.make_cov_psd(torch.from_numpy(ns.copy())).numpy()
        neg = -spd                              # |.| repairs it (Q2)
        out["d_in"] = neg
        out["d_out"] = tm.make_cov_psd(torch.from_numpy(neg.copy())).numpy()
        r5 = A[:, :5] @ A[:, :5].T              # rank 5 with mixed signs: ends on the diagonal fallback
        r5 = 0.5 * (r5 + r5.T)
        out["e_in"] = r5
        out["e_out"] = tm.make_cov_psd(torch.from_numpy(r5.copy())).numpy()
    np.savez_compressed(os.path.join(HERE, "psd.npz"), **out)


def gen_tanimoto():
    src = open("/root/reference/SOBER/_drug_modelling.py").read()
    start = src.index("def batch_tanimoto_sim")
    end = src.index("class BitDistance")
    ns = {"torch": torch}
    exec(src[start:end], ns)            # the function is plain torch
    f = ns["batch_tanimoto_sim"]
    rng = np.random.default_rng(400)
    x1 = (rng.random((20, 96)) < 0.2).astype(np.float64)
    x2 = (rng.random((35, 96)) < 0.2).astype(np.float64)
    x3 = (rng.random((4, 9, 96)) < 0.2).astype(np.float64)
    x2[0] = 0.0
    x1[0] = 0.0
    out = dict(x1=x1, x2=x2, x3=x3,
               k12=f(torch.from_numpy(x1), torch.from_numpy(x2)).numpy(),
               k13=f(torch.from_numpy(x1), torch.from_numpy(x3)).numpy())
    np.savez_compressed(os.path.join(HERE, "tanimoto.npz"), **out)


def gen_kernel_calls(ref):
    """Kernel.__call__ in all three modes with 2-D and 3-D second argument."""
    out = {}
    for kind in (O.RBF, O.MATERN52, O.TANIMOTO):
        case = dict(kind=kind, N=60, M=12, d=16 if kind == O.TANIMOTO else 3, n_obs=9, seed=500,
                    ard=True, mean_const=0.5, outputscale=1.3)
        inp = synth(case)
        spec = build_spec(case, inp)
        model = DuckModel(spec)
        x = torch.from_numpy(inp["X_nys"])
        y2 = torch.from_numpy(inp["X_cand"][:40])
        y3 = torch.from_numpy(inp["X_cand"][:40]).reshape(5, 8, -1)
        out.update({f"{kind}_X_obs": inp["X_obs"], f"{kind}_S_cache": spec.S_cache.numpy(),
                    f"{kind}_alpha": spec.alpha.numpy(), f"{kind}_ls": spec.lengthscale.numpy(),
                    f"{kind}_x": x.numpy(), f"{kind}_y2": y2.numpy()})
        for mode in O.Kernel.MODES:
            k = ref["_kernel"].Kernel(model, mode=mode)
            out[f"{kind}_{mode}_2d"] = k(x, y2).numpy()
            out[f"{kind}_{mode}_3d"] = k(x, y3).numpy()
    np.savez_compressed(os.path.join(HERE, "kernel_calls.npz"), **out)


def gen_pi(ref):
    """PI.lfi / PI.__call__ of SOBER/_pi.py and predict of SOBER/_gp.py:212-238 through the duck model."""
    import torch as _torch
    ref["_pi"].torch = _torch                 # _pi.py uses torch without importing it
    out = {}
    for kind in (O.RBF, O.MATERN52, O.TANIMOTO):
        case = dict(kind=kind, N=400, M=10, d=24 if kind == O.TANIMOTO else 4, n_obs=15, seed=600, ard=True,
                    mean_const=0.25, outputscale=1.4)
        inp = synth(case)
        spec = build_spec(case, inp)
        model = DuckModel(spec)
        pi = ref["_pi"].PI(model, label="lfi")
        X = torch.from_numpy(inp["X_cand"])
        mean, var = ref["_gp"].predict(X, model)
        out.update({f"{kind}_X": inp["X_cand"], f"{kind}_X_obs": inp["X_obs"], f"{kind}_S_cache": spec.S_cache.numpy(),
                    f"{kind}_alpha": spec.alpha.numpy(), f"{kind}_ls": spec.lengthscale.numpy(),
                    f"{kind}_mean": mean.numpy(), f"{kind}_var": var.numpy(), f"{kind}_eta": pi.eta,
                    f"{kind}_lfi": pi(X).numpy(), f"{kind}_loglfi": pi(X, log=True).numpy()})
    np.savez_compressed(os.path.join(HERE, "pi.npz"), **out)


def gen_wkde(ref):
    """WeightedKernelDensityEstimation of SOBER/_wkde.py: construction (seeded) + pdf, with and without bounds."""
    import abc
    prior = types.ModuleType("SOBER._prior")
    TM = ref["_utils"].TensorManager

    class BasePrior(abc.ABC, TM):                      # SOBER/_prior.py:12-24 needs _tmvn/mvnorm: stub the base only
        def __init__(self):
            TM.__init__(self)
    prior.BasePrior = BasePrior
    sys.modules["SOBER._prior"] = prior
    mv = types.ModuleType("SOBER.mvnorm")
    mv.multivariate_normal_cdf = None
    sys.modules["SOBER.mvnorm"] = mv
    spec = importlib.util.spec_from_file_location("SOBER._wkde", f"{REF}/_wkde.py")
    m = importlib.util.module_from_spec(spec)
    sys.modules["SOBER._wkde"] = m
    spec.loader.exec_module(m)
    rng = np.random.default_rng(700)
    out = {}
    for tag, d, n, n_kde, bounded in (("a", 3, 3000, 256, True), ("b", 5, 800, 4096, False)):
        X = rng.random((n, d))
        W = rng.random(n) ** 3
        bounds = torch.tensor([[0.0] * d, [1.0] * d], dtype=torch.double) if bounded else None
        torch.manual_seed(11)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            kde = m.WeightedKernelDensityEstimation(torch.from_numpy(X.copy()), torch.from_numpy(W.copy()), d,
                                                    bounds=bounds, n_kde=n_kde)
            Xq = rng.random((500, d)) * 1.2 - 0.1
            pdf = kde.pdf(torch.from_numpy(Xq))
            n_rec = 2000 if bounded else 1500
            torch.manual_seed(5)
            smp = kde.sample(n_rec)                       # SOBER/_wkde.py:221-248, CPU generator
        out.update({f"{tag}_X": X, f"{tag}_W": W, f"{tag}_n_kde": n_kde, f"{tag}_bounded": bounded,
                    f"{tag}_Xobs": kde.Xobs.numpy(), f"{tag}_weights": kde.weights.numpy(),
                    f"{tag}_cov": kde.covariance.numpy(), f"{tag}_bw": float(kde.bw), f"{tag}_Xq": Xq,
                    f"{tag}_pdf": pdf.numpy(), f"{tag}_n_rec": n_rec, f"{tag}_sample": smp.numpy()})
    np.savez_compressed(os.path.join(HERE, "wkde.npz"), **out)


def gen_basq(ref):
    """BASQ provider: ScaleMmltGP.gspace_kernel / gspace_mean_predict
    (SOBER/BASQ/_scale_mmlt.py:206-275) and BASQ.quadrature (SOBER/BASQ/_basq.py:43-81) run from the
    reference's own methods.  ScaleMmltGP.__init__ trains a gpytorch model (not installed), so the
    instance is created without it and given the duck-typed GP; BASQ likewise gets a fixed prior sample."""
    pkg = types.ModuleType("SOBER.BASQ")
    pkg.__path__ = [f"{REF}/BASQ"]
    sys.modules["SOBER.BASQ"] = pkg
    spec_ = importlib.util.spec_from_file_location("SOBER.BASQ._scale_mmlt", f"{REF}/BASQ/_scale_mmlt.py")
    sm = importlib.util.module_from_spec(spec_)
    sys.modules["SOBER.BASQ._scale_mmlt"] = sm
    spec_.loader.exec_module(sm)
    smp = types.ModuleType("SOBER._sampler")                # _basq.py imports MixtureSampler only to build it
    smp.MixtureSampler = lambda *a, **k: None
    sys.modules["SOBER._sampler"] = smp
    spec_ = importlib.util.spec_from_file_location("SOBER.BASQ._basq", f"{REF}/BASQ/_basq.py")
    bq = importlib.util.module_from_spec(spec_)
    sys.modules["SOBER.BASQ._basq"] = bq
    spec_.loader.exec_module(bq)

    out = {}
    for tag, kind, d, n_obs, N, M, b, seed in (("a", O.RBF, 4, 40, 4000, 80, 12, 21),
                                               ("b", O.MATERN52, 3, 30, 2500, 64, 10, 22)):
        rng = np.random.default_rng(seed)
        X_obs = rng.random((n_obs, d))
        ls = 0.35 * (1.0 + np.arange(d) / d)
        y_h = np.log(np.exp(-8.0 * ((X_obs - 0.5) ** 2).sum(1)) + 1.0) * 3.0       # h-space observations
        spec = O.make_spec(kind, torch.from_numpy(X_obs), torch.from_numpy(ls), outputscale=1.3, noise=1e-3,
                           mean_const=0.15, y_obs=torch.from_numpy(y_h))
        g = object.__new__(sm.ScaleMmltGP)
        ref["_utils"].Utils.__init__(g)
        g.model = DuckModel(spec)
        g.jitter = g.tensor(0)
        g.beta = torch.tensor(-3.25, dtype=torch.double)
        X_cand = rng.random((N, d))
        Xc = torch.from_numpy(X_cand)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            K2 = g.gspace_kernel(Xc[:10], Xc[100:150])
            K3 = g.gspace_kernel(Xc[:10], Xc[200:260].reshape(3, 20, d))
            mug = g.gspace_mean_predict(Xc[:100])
            mug2, varg = g.gspace_predict(Xc[:100])
            basq = object.__new__(bq.BASQ)
            ref["_utils"].TensorManager.__init__(basq)
            basq.prior = types.SimpleNamespace(sample=lambda n: Xc[:n])
            basq.kernel, basq.pred_mean, basq.beta = g.gspace_kernel, g.gspace_mean_predict, g.beta
            torch.manual_seed(SEED_CALL)
            with contextlib.redirect_stdout(None):
                ELML, AVLML = basq.quadrature(N, M, b)
            # the same recombination once more to store its indices and weights
            torch.manual_seed(SEED_CALL)
            w_IS = torch.ones(N, dtype=torch.double) / N
            idx, w = ref["_rchq"].recombination(Xc, Xc[:M], b, g.gspace_kernel, torch.device("cpu"), torch.double,
                                                init_weights=w_IS)
        out.update({f"{tag}_kind": kind, f"{tag}_X_obs": X_obs, f"{tag}_ls": ls, f"{tag}_alpha": spec.alpha.numpy(),
                    f"{tag}_S_cache": spec.S_cache.numpy(), f"{tag}_X_cand": X_cand, f"{tag}_M": M, f"{tag}_b": b,
                    f"{tag}_K2": K2.numpy(), f"{tag}_K3": K3.numpy(), f"{tag}_mug": mug.numpy(),
                    f"{tag}_varg": varg.numpy(), f"{tag}_ELML": ELML, f"{tag}_AVLML": AVLML,
                    f"{tag}_idx": idx.numpy(), f"{tag}_w": w.numpy(), f"{tag}_EML": float(basq.EML)})
        print(f"basq {tag}: |idx|={len(idx)} ELML={ELML:.6f} AVLML={AVLML:.6f}")
    np.savez_compressed(os.path.join(HERE, "basq.npz"), **out)


def gen_pruning(ref):
    """EmpiricalSampler.adaptive_pruning of SOBER/_sampler.py:325-349 (it does not touch `self`): every branch."""
    import types
    for name, names in (("SOBER._prior", ("Uniform", "BinaryPrior", "CategoricalPrior", "MixedBinaryPrior",
                                          "MixedCategoricalPrior")),
                        ("SOBER._prior_update", ("update_mixed_prior", "update_binary_prior",
                                                 "update_categorical_prior", "update_continuous_prior"))):
        m = types.ModuleType(name)
        for n in names:
            setattr(m, n, object)
        sys.modules[name] = m
    spec = importlib.util.spec_from_file_location("SOBER._sampler", f"{REF}/_sampler.py")
    smp = importlib.util.module_from_spec(spec)
    sys.modules["SOBER._sampler"] = smp
    spec.loader.exec_module(smp)
    fn = smp.EmpiricalSampler.adaptive_pruning
    g = torch.Generator().manual_seed(3)
    out = {}
    cases = [("many_above", torch.rand(5000, generator=g, dtype=torch.double), 1000, 100),      # n_accepted >= n_rec
             ("few_above", torch.rand(5000, generator=g, dtype=torch.double) * 1.02e-3, 1000, 300),   # n_nys >= n_accepted
             ("between", torch.rand(5000, generator=g, dtype=torch.double) * 1.2e-3, 2000, 100),      # n_accepted kept
             ("none_above", torch.rand(500, generator=g, dtype=torch.double) * 1e-4, 100, 20)]        # except branch
    for tag, w, n_rec, n_nys in cases:
        idx = fn(None, w, n_rec, n_nys)
        out[f"{tag}_w"], out[f"{tag}_idx"] = w.numpy(), idx.numpy()
        out[f"{tag}_args"] = np.array([n_rec, n_nys])
        print(f"pruning {tag}: kept {len(idx)} of {len(w)}")
    np.savez_compressed(os.path.join(HERE, "pruning.npz"), **out)


D1_CASE = dict(kind=O.RBF, mode="predictive_covariance", N=1000, M=90, d=1, b=16, n_obs=40, seed=106, ard=True,
               mean_const=0.4)
# the same input with a pool that halves without leftovers (1024 = 32 * 2^5): there the recombination step preserves
# the integrals of its test functions EXACTLY (the leftover quirk Q1 is what breaks that at N = 1000), which gives a
# criterion that does not depend on which of several equally valid point sets an implementation lands on
D1_EXACT_CASE = dict(D1_CASE, N=1024)


def gen_d1_sensitivity(ref):
    """One-dimensional inputs: 90 Nystrom points on a line give a Gram matrix of numerical rank ~17 for 15 test
    functions, and the reference's OWN weights then move by ~1e-3 when the candidate coordinates change by one ulp
    (same selected indices).  That self-sensitivity -- not 1e-4 -- is what any second implementation can be held to
    on this input; recorded here from the reference itself (three one-ulp perturbations)."""
    case = D1_CASE
    inp = synth(case)
    base = run_reference(ref, case, inp, threads=1)
    rng = np.random.default_rng(0)
    deltas, same = [], []
    for _ in range(3):
        inp2 = dict(inp)
        inp2["X_cand"] = inp["X_cand"] * (1.0 + 2.2e-16 * rng.integers(-1, 2, size=inp["X_cand"].shape))
        r2 = run_reference(ref, case, inp2, threads=1)
        same.append(bool(torch.equal(r2["idx"], base["idx"])))
        deltas.append(float(((r2["w"] - base["w"]).abs() / base["w"].abs()).max()) if same[-1] else np.nan)
    print("d = 1: reference under one-ulp perturbations: same indices", same, "max rel weight change", deltas)
    np.savez_compressed(os.path.join(HERE, "d1_sensitivity.npz"), idx=base["idx"].numpy(), w=base["w"].numpy(),
                        same_idx=np.array(same), rel_w_change=np.array(deltas))
    exact = run_reference(ref, D1_EXACT_CASE, synth(D1_EXACT_CASE), threads=1)
    np.savez_compressed(os.path.join(HERE, "d1_exact.npz"), idx=exact["idx"].numpy(), w=exact["w"].numpy())


def load_sampler_sober(ref):
    """SOBER/_sampler.py and SOBER/_sober.py from their own files.  The prior machinery around the path (`_prior.py`,
    `_prior_update.py`: truncated MVNs, WKDE refits) is not under test: empty stand-ins for the import lines, and
    `update_continuous_prior` keeps the prior as it is."""
    ref["_pi"].torch = torch                       # _pi.py uses torch without importing it
    prior = types.ModuleType("SOBER._prior")
    for n in ("Uniform", "BinaryPrior", "CategoricalPrior", "MixedBinaryPrior", "MixedCategoricalPrior"):
        setattr(prior, n, type(n, (), {}))
    sys.modules["SOBER._prior"] = prior
    upd = types.ModuleType("SOBER._prior_update")
    upd.update_mixed_prior = upd.update_binary_prior = upd.update_categorical_prior = None
    upd.update_continuous_prior = lambda X, w, prior, n_dims: prior
    sys.modules["SOBER._prior_update"] = upd
    for name in ("PI_FBGP", "PI_BQ"):              # imported by name in _sober.py (other model families)
        if not hasattr(ref["_pi"], name):
            setattr(ref["_pi"], name, None)
    for name in ("_sampler", "_sober"):
        spec = importlib.util.spec_from_file_location(f"SOBER.{name}", f"{REF}/{name}.py")
        m = importlib.util.module_from_spec(spec)
        sys.modules[f"SOBER.{name}"] = m
        spec.loader.exec_module(m)
        ref[name] = m
    return ref


class DatasetPrior:
    type = "dataset"

    def __init__(self, X):
        self.X = X

    def available_candidates(self):
        return self.X


class UniformPrior:
    """Unit-cube prior with the three members `sampling_candidates` touches; draws on the CPU generator."""
    type = "continuous"

    def __init__(self, d, device=None):
        self.n_dims, self.device = d, device
        self.bounds = torch.stack([torch.zeros(d, dtype=torch.double), torch.ones(d, dtype=torch.double)])

    def sample(self, n):
        x = torch.rand(n, self.n_dims, dtype=torch.double)
        return x if self.device is None else x.to(self.device)

    def pdf(self, X):
        return torch.ones(len(X), dtype=torch.double, device=X.device)


SOBER_CASES = {
    "dataset": dict(kind=O.TANIMOTO, N=64, M=8, d=64, n_obs=20, seed=77, mean_const=0.2,
                    kernel_type="weighted_predictive_covariance", pool_seed=3, pool_n=900, pool_p=0.1,
                    n_rec=600, n_nys=40, batch=8, seed_call=123),
    "continuous": dict(kind=O.RBF, N=64, M=8, d=3, n_obs=15, seed=78, mean_const=0.2,
                       kernel_type="predictive_covariance", n_rec=1500, n_nys=48, batch=8, seed_call=321),
}


def sober_model(case):
    inp = synth(case)
    spec = build_spec(case, inp)
    model = DuckModel(spec)
    model.train_targets = torch.zeros(case["n_obs"], dtype=torch.double)
    return model, spec


def gen_sober(ref):
    """`Sober.next_batch` of SOBER/_sober.py:125-195 with its three return shapes: (w_rchq, X_batch) |
    (idx_rchq, X_batch) on a dataset prior with and without pruning | X_batch on a sampled (continuous) prior."""
    load_sampler_sober(ref)
    out = {}
    c = SOBER_CASES["dataset"]
    rng = np.random.default_rng(c["pool_seed"])
    pool = torch.from_numpy((rng.random((c["pool_n"], c["d"])) < c["pool_p"]).astype(np.float64))
    model, _ = sober_model(c)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        for pruning in (True, False):
            for rw in (False, True):
                sober = ref["_sober"].Sober(DatasetPrior(pool), model, kernel_type=c["kernel_type"],
                                            dataset_pruning=pruning)
                torch.manual_seed(c["seed_call"])
                a, Xb = sober.next_batch(c["n_rec"], c["n_nys"], c["batch"], return_weights=rw)
                tag = f"dataset_p{int(pruning)}_w{int(rw)}"
                out[tag + "_first"], out[tag + "_X"] = a.numpy(), Xb.numpy()
                print(tag, a.shape, Xb.shape)
        c = SOBER_CASES["continuous"]
        model, _ = sober_model(c)
        sober = ref["_sober"].Sober(UniformPrior(c["d"]), model, kernel_type=c["kernel_type"])
        torch.manual_seed(c["seed_call"])
        Xb = sober.next_batch(c["n_rec"], c["n_nys"], c["batch"])
        out["continuous_X"] = Xb.numpy()
        print("continuous", Xb.shape)
    np.savez_compressed(os.path.join(HERE, "sober_next_batch.npz"), **out)


def gen_kmeans_screened(ref):
    """The reference's KMeans (SOBER/_weights.py:100-126) on shapes whose E step the device runs SCREENED by default
    (BF16 matrix cores + exact FP64 re-check, csrc/kmeans.hip: N * ceil((d + 1) / 4) >= 300000): 120000 x 10 into 64
    clusters -- the reference's (N, K, D) temporary is 614 MB --, once on the unit cube and once on the same pool moved
    by 1e4 (the screen works on centred coordinates).  Only the seed, the labels (one byte each) and the centroids are
    stored."""
    KMeans = ref["_weights"].KMeans
    out = {}
    N, d, K, seed = 120000, 10, 64, 321
    x = np.random.default_rng(seed).random((N, d))
    for tag, off in (("unit", 0.0), ("offset", 1e4)):
        xv = x + off
        cl, c = KMeans(torch.from_numpy(xv.copy()), K=K)
        out.update({f"{tag}_off": off, f"{tag}_cl": cl.numpy().astype(np.uint8), f"{tag}_c": c.numpy(),
                    f"{tag}_cks_x": checksum(xv)})
        print("kmeans_screened", tag, "cluster sizes", np.bincount(cl.numpy(), minlength=K).min(), "...",
              np.bincount(cl.numpy(), minlength=K).max())
    out.update(seed=seed, N=N, d=d, K=K)
    np.savez_compressed(os.path.join(HERE, "kmeans_screened.npz"), **out)


def fuzz_cases():
    """The 64 seeded random recombination cases of tests/test_oracle_vs_reference_fuzz.py: kinds x modes x leftovers of
    every kind x calc_obj x zero weights x ARD (inputs from synth(case), so only the cases' parameters are code)."""
    rng = np.random.default_rng(20261003)
    kinds = [O.RBF, O.MATERN52, O.TANIMOTO]
    modes = ["predictive_covariance", "weighted_predictive_covariance", "kernel"]
    out = []
    for i in range(64):
        kind = kinds[i % 3] if i % 8 != 7 else O.TANIMOTO
        mode = modes[(i // 3) % 3]
        b = int(rng.integers(4, 25))
        # leftovers of every kind: R mod 2b in {0, 1, 2b-1, random}, pools below one level (straight to the final level),
        # pools of exactly one level
        shape = i % 6
        S = 2 * b
        E = int(rng.integers(2, 30))
        N = {0: E * S, 1: E * S + 1, 2: E * S + S - 1, 3: E * S + int(rng.integers(1, S)),
             4: int(rng.integers(b + 1, S + 1)), 5: S + int(rng.integers(1, S))}[shape]
        d = int(rng.integers(2, 9)) if kind != O.TANIMOTO else int(rng.choice([64, 96, 128, 200]))
        M = int(rng.integers(max(b + 2, 20), 90))
        M = min(M, N)
        case = dict(name=f"fuzz{i}", kind=kind, mode=mode, N=N, M=M, d=d, b=b, n_obs=int(rng.integers(5, 40)),
                    seed=1000 + i, ard=bool(rng.integers(0, 2)) and kind != O.TANIMOTO,
                    zero_frac=0.25 if i % 5 == 0 else 0.0, calc_obj=(i % 4 == 1),
                    outputscale=float(rng.uniform(0.5, 2.0)), mean_const=float(rng.uniform(0.2, 1.0)),
                    bit_p=float(rng.uniform(0.05, 0.3)))
        if M < b + 1:
            continue
        out.append(case)
    return out


def gen_reference_fuzz(ref):
    """The reference's recombination (run_reference, one thread) on every case of fuzz_cases(): indices, weights and the
    mutated init_weights, or the reference's own exception where it cannot run the input.  The inputs' checksums are
    stored beside them, so that a change of synth() shows up as such and not as a parity failure."""
    out = {}
    for case in fuzz_cases():
        n = case["name"]
        inp = synth(case)
        out[f"{n}_cks_x"] = checksum(inp["X_cand"])
        try:
            rec = run_reference(ref, case, inp, threads=1)
        except Exception as e:                       # noqa: BLE001  (e.g. a singular step)
            out[f"{n}_raised"] = np.array(f"{type(e).__name__}: {e}")
            print(n, "reference raised", type(e).__name__)
            continue
        out[f"{n}_idx"], out[f"{n}_w"], out[f"{n}_mu_after"] = rec["idx"].numpy(), rec["w"].numpy(), rec["mu_after"].numpy()
        print(n, case["kind"], case["mode"], "N", case["N"], "b", case["b"], "->", len(rec["idx"]))
    np.savez_compressed(os.path.join(HERE, "reference_fuzz.npz"), **out)


DROPIN_SAMPLER_CASES = ("cfg1_rbf_ard", "rbf_b30", "matern_b20", "tanimoto_weighted", "rbf_zero_weights")


def _record_call(store, tag, args, kwargs):
    """One call of the reference into `recombination`: how it is made (which arguments positional, which by keyword,
    device and dtype) and its tensors; the CPU generator's state in front of it (the svd_lowrank draw)."""
    store[f"{tag}_n_args"] = np.array(len(args))
    store[f"{tag}_kwargs"] = np.array(sorted(kwargs))
    X_cand, X_nys, b, _kernel, device, dtype = args
    store[f"{tag}_X_cand"], store[f"{tag}_X_nys"] = X_cand.numpy().copy(), X_nys.numpy().copy()
    store[f"{tag}_b"] = np.array(b)
    store[f"{tag}_device"], store[f"{tag}_dtype"] = np.array(str(device)), np.array(str(dtype))
    store[f"{tag}_init_weights"] = kwargs["init_weights"].numpy().copy()
    store[f"{tag}_calc_obj_none"] = np.array(kwargs.get("calc_obj") is None)
    store[f"{tag}_rng_state"] = torch.get_rng_state().numpy().copy()


def gen_dropin(ref):
    """The reference's own callers of the hot path, recorded: `RecombinationSampler.sampling_recombination`
    (SOBER/_sampler.py:27-59) on the DROPIN_SAMPLER_CASES goldens, and `Sober.next_batch` (SOBER/_sober.py:125-195) in
    the scenarios of sober_next_batch.npz (dataset prior with / without pruning and with / without return_weights; a
    sampled prior).  For every call into `recombination`: the call as made, the generator state in front of it, its
    result and the mutated init_weights; for every `Kernel(...)` the reference's `Sober` builds: positional count and
    keywords; for `Sober.next_batch`: its return values and, with pruning, the kept candidates' pool indices.  And the
    reference's `Sober.should_reset_prior` verdicts on the seeded observation histories of
    tests/test_dropin_reference.py::test_should_reset_prior_equals_the_reference."""
    load_sampler_sober(ref)
    out = {}
    calls = []
    orig_rec, orig_kernel = ref["_sampler"].recombination, ref["_sober"].Kernel

    def rec_wrap(*args, **kwargs):
        tag = f"call{len(calls)}"
        _record_call(out, tag, args, kwargs)
        idx, w = orig_rec(*args, **kwargs)
        out[f"{tag}_idx"], out[f"{tag}_w"] = idx.numpy().copy(), w.numpy().copy()
        out[f"{tag}_mu_after"] = kwargs["init_weights"].numpy().copy()
        calls.append(tag)
        return idx, w

    kernel_call = {}

    def kernel_wrap(*args, **kwargs):
        kernel_call.update(n_args=np.array(len(args)), kwargs=np.array(sorted(kwargs)),
                           mode=np.array(kwargs.get("mode", args[1] if len(args) > 1 else "")))
        return orig_kernel(*args, **kwargs)

    def keep_kernel_call(tag):
        for k, v in kernel_call.items():
            out[f"{tag}_kernel_{k}"] = v
        kernel_call.clear()

    ref["_sampler"].recombination, ref["_sober"].Kernel = rec_wrap, kernel_wrap
    try:
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            for name in DROPIN_SAMPLER_CASES:
                case, inp, spec, z = load_case(os.path.join(HERE, f"recomb_{name}.npz"))
                sampler = ref["_sampler"].RecombinationSampler(ref["_kernel"].Kernel(DuckModel(spec), mode=case["mode"]))
                torch.manual_seed(SEED_CALL)
                sampler.sampling_recombination(torch.from_numpy(inp["X_cand"].copy()), torch.from_numpy(inp["X_nys"].copy()),
                                               torch.from_numpy(inp["mu0"].copy()), case["b"])
                out[f"sampler_{name}_call"] = np.array(calls[-1])
                assert np.array_equal(out[f"{calls[-1]}_idx"], z["idx"]), name
                print("sampler", name, calls[-1])
            c = SOBER_CASES["dataset"]
            rng = np.random.default_rng(c["pool_seed"])
            pool = torch.from_numpy((rng.random((c["pool_n"], c["d"])) < c["pool_p"]).astype(np.float64))
            model, _ = sober_model(c)
            for pruning in (True, False):
                for rw in (False, True):
                    tag = f"dataset_p{int(pruning)}_w{int(rw)}"
                    sober = ref["_sober"].Sober(DatasetPrior(pool), model, kernel_type=c["kernel_type"],
                                                dataset_pruning=pruning)
                    keep_kernel_call(tag)
                    orig_sd = sober.sampling_datasets

                    def sd_wrap(n_rec, n_nys, _orig=orig_sd, _tag=tag):
                        em = _orig(n_rec, n_nys)
                        if len(em) == 4:
                            out[f"{_tag}_idx_sampled"] = em[0].numpy().copy()
                        return em
                    sober.sampling_datasets = sd_wrap
                    torch.manual_seed(c["seed_call"])
                    a, Xb = sober.next_batch(c["n_rec"], c["n_nys"], c["batch"], return_weights=rw)
                    out[f"{tag}_call"], out[f"{tag}_first"], out[f"{tag}_X"] = np.array(calls[-1]), a.numpy(), Xb.numpy()
                    print(tag, calls[-1], a.shape, Xb.shape)
            c = SOBER_CASES["continuous"]
            model, _ = sober_model(c)
            sober = ref["_sober"].Sober(UniformPrior(c["d"]), model, kernel_type=c["kernel_type"])
            keep_kernel_call("continuous")
            torch.manual_seed(c["seed_call"])
            Xb = sober.next_batch(c["n_rec"], c["n_nys"], c["batch"])
            out["continuous_call"], out["continuous_X"] = np.array(calls[-1]), Xb.numpy()
            print("continuous", calls[-1], Xb.shape)
    finally:
        ref["_sampler"].recombination, ref["_sober"].Kernel = orig_rec, orig_kernel
    out["reset_verdicts"] = np.array(reset_verdicts(ref["_sober"].Sober))
    print("should_reset_prior", int(out["reset_verdicts"].sum()), "of", out["reset_verdicts"].size)
    np.savez_compressed(os.path.join(HERE, "dropin_calls.npz"), **out)


def reset_histories():
    """Seeded observation histories for `should_reset_prior` (SOBER/_sober.py:84-123): (n_init, batch_size, y) x 300,
    each asked with recycle_prior True and False."""
    rng = np.random.default_rng(5)
    out = []
    for _ in range(300):
        n_init = int(rng.integers(1, 12))
        bs = int(rng.integers(1, 9))
        n_batches = int(rng.integers(0, 7))
        extra = int(rng.integers(0, bs)) if n_batches and rng.random() < 0.3 else 0
        y = torch.from_numpy(rng.standard_normal(n_init + n_batches * bs + extra))
        if rng.random() < 0.3:                                           # a maximum early in the history
            y[int(rng.integers(0, n_init))] = 10.0
        out.append((n_init, bs, y))
    return out


def reset_verdicts(SoberCls):
    """`should_reset_prior` of the reference's `Sober` on reset_histories(): a (300, 2) bool array, recycle True / False."""
    res = []
    for n_init, bs, y in reset_histories():
        model = types.SimpleNamespace(train_targets=y)
        row = []
        for recycle in (True, False):
            a = object.__new__(SoberCls)
            a.fbgp, a.is_bq, a.n_init, a.n_batches_until_reset = False, False, n_init, 3
            a.pi = types.SimpleNamespace(model=model)
            a.tensor = torch.tensor
            row.append(bool(a.should_reset_prior(bs, recycle)))
        res.append(row)
    return res


if __name__ == "__main__":
    # python make_golden.py [recombination kmeans kmeans_screened weights psd tanimoto kernel_calls pi wkde basq pruning sober d1 reference_fuzz dropin]   (default: all)
    ref = load_reference()
    gens = {"recombination": gen_recombination, "kmeans": gen_kmeans, "kmeans_screened": gen_kmeans_screened, "weights": gen_weights, "psd": gen_psd,
            "tanimoto": lambda ref: gen_tanimoto(), "kernel_calls": gen_kernel_calls, "pi": gen_pi,
            "wkde": gen_wkde, "basq": gen_basq, "pruning": gen_pruning, "sober": gen_sober, "d1": gen_d1_sensitivity,
            "reference_fuzz": gen_reference_fuzz, "dropin": gen_dropin}
    for name in (sys.argv[1:] or list(gens)):
        gens[name](ref)
    tot = sum(os.path.getsize(os.path.join(HERE, f)) for f in os.listdir(HERE) if f.endswith(".npz"))
    print(f"total fixture size {tot / 1e6:.2f} MB")
