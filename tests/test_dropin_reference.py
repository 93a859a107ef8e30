"""Drop-in proof against the reference's OWN callers, replayed from a recording (tests/golden/dropin_calls.npz, written
by tests/golden/make_golden.py:gen_dropin from the reference's code; tests/test_hip_parity.py::
test_sober_next_batch_vs_reference replays the same scenarios through the product's `Sober` on the device).

The reference's `RecombinationSampler` (SOBER/_sampler.py:11-59) and `Sober` (SOBER/_sober.py:9-195) reach the hot path
through two names: `recombination(X_cand, X_nys, batch_size, kernel, device, dtype, init_weights=..., calc_obj=...)`
and `Kernel(model, mode=...)`.  The recording holds every such call they made -- which arguments positional, which by
keyword, the tensors, the CPU generator's state in front of it -- with what the reference returned.  Here each call is
made again, the same way, to `sober_amd.recombination` with a `sober_amd.Kernel` (and with them `RecombinationEngine`,
the host logic of the product); without a GPU the bulk kernels behind `recombination` are the CPU test double
(tests/_oracle_ops.py).  Checked: the reference's callers get the reference's results through the swapped functions,
for `sampling_recombination` and for the three return shapes of `Sober.next_batch`."""
import os
import warnings

import numpy as np
import pytest
import torch

import sober_amd
from tests._oracle_ops import OracleOps
from tests.golden import make_golden as MG
from tests.golden.synth import build_spec, load_case, synth

GOLD = os.path.join(os.path.dirname(__file__), "golden")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(GOLD, "dropin_calls.npz"))


def _ours(*a, **k):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return sober_amd.recombination(*a, **k, _ops=OracleOps())


def _replay(ref, tag, kernel):
    """The recorded call `tag` made again to sober_amd.recombination, as the reference's caller made it (same positional
    / keyword split, same generator state) -> (idx, w, init_weights after the call)."""
    assert int(ref[f"{tag}_n_args"]) == 6
    assert list(ref[f"{tag}_kwargs"]) == ["calc_obj", "init_weights"] and bool(ref[f"{tag}_calc_obj_none"])
    assert str(ref[f"{tag}_dtype"]) == "torch.float64"
    mu = _t(ref[f"{tag}_init_weights"].copy())
    args = (_t(ref[f"{tag}_X_cand"]), _t(ref[f"{tag}_X_nys"]), int(ref[f"{tag}_b"]), kernel,
            torch.device(str(ref[f"{tag}_device"])), torch.double)
    torch.set_rng_state(_t(ref[f"{tag}_rng_state"]))
    idx, w = _ours(*args, init_weights=mu, calc_obj=None)
    return idx, w, mu


@pytest.mark.parametrize("name", list(MG.DROPIN_SAMPLER_CASES))
def test_reference_sampler_with_swapped_recombination(ref, name):
    """SOBER/_sampler.py:27-59 calling sober_amd.recombination with a sober_amd.Kernel: the reference golden."""
    case, inp, spec, z = load_case(os.path.join(GOLD, f"recomb_{name}.npz"))
    ks = sober_amd.KernelSpec(spec.kind, spec.lengthscale, spec.outputscale, spec.X_obs, spec.S_cache, spec.noise,
                              spec.mean_const, spec.alpha)
    tag = str(ref[f"sampler_{name}_call"])
    assert np.array_equal(ref[f"{tag}_X_cand"], inp["X_cand"]) and np.array_equal(ref[f"{tag}_init_weights"], inp["mu0"])
    assert int(ref[f"{tag}_b"]) == case["b"]
    idx, w, w0 = _replay(ref, tag, sober_amd.Kernel(ks, case["mode"]))
    assert np.array_equal(idx.numpy(), z["idx"])
    np.testing.assert_allclose(w.numpy(), z["w"], rtol=1e-9)
    nz = torch.nonzero(w0).flatten().numpy()
    assert np.array_equal(nz, z["mu_after_idx"])                            # Q3 through the reference's caller
    assert np.array_equal(nz, np.flatnonzero(ref[f"{tag}_mu_after"]))


def _kernel(ref, case, tag):
    """sober_amd.Kernel built as the reference's `Sober` builds its Kernel (the recorded call: the model, mode= by
    keyword) from a model of the recorded scenario."""
    inp = synth(case)
    spec = build_spec(case, inp)
    model = MG.DuckModel(spec)
    model.train_targets = torch.zeros(case["n_obs"], dtype=torch.double)
    # (a gpytorch model is read by its class names, sober_amd/_kernel.py:spec_from_model; the duck model of the
    #  fixtures has none, so it carries the spec itself)
    model.kernel_spec = sober_amd.KernelSpec(spec.kind, spec.lengthscale, spec.outputscale, spec.X_obs, spec.S_cache,
                                             spec.noise, spec.mean_const, spec.alpha)
    assert int(ref[f"{tag}_kernel_n_args"]) == 1 and list(ref[f"{tag}_kernel_kwargs"]) == ["mode"]
    assert str(ref[f"{tag}_kernel_mode"]) == case["kernel_type"]
    return sober_amd.Kernel(model, mode=case["kernel_type"])


@pytest.mark.parametrize("pruning", [True, False])
def test_reference_sober_next_batch_dataset_prior(ref, pruning):
    """`Sober.next_batch` on a dataset prior (SOBER/_sober.py:158-195), both dataset return shapes and the
    return_weights shape: swapped == unswapped."""
    c = MG.SOBER_CASES["dataset"]
    for rw in (False, True):
        tag = f"dataset_p{int(pruning)}_w{int(rw)}"
        kernel = _kernel(ref, c, tag)
        call = str(ref[f"{tag}_call"])
        assert int(ref[f"{call}_b"]) == c["batch"]
        idx, w, _ = _replay(ref, call, kernel)
        X_batch = _t(ref[f"{call}_X_cand"])[idx]                            # SOBER/_sober.py:181
        if rw:                                                              # (w_rchq, X_batch)
            np.testing.assert_allclose(w.numpy(), ref[f"{tag}_first"], rtol=1e-9)
        else:                                                               # (idx_rchq, X_batch)
            if pruning:                                                     # indices into the prior's available rows
                idx = _t(ref[f"{tag}_idx_sampled"])[idx]
            assert idx.dtype == torch.int64 and np.array_equal(idx.numpy(), ref[f"{tag}_first"])
        assert np.array_equal(X_batch.numpy(), ref[f"{tag}_X"])


def test_reference_sober_next_batch_sampled_prior(ref):
    """The third return shape (X_batch alone) through `sampling_candidates` (SOBER/_sampler.py:264-323, KMeans
    Nystrom subsample for a continuous prior): swapped == unswapped."""
    c = MG.SOBER_CASES["continuous"]
    call = str(ref["continuous_call"])
    idx, _, _ = _replay(ref, call, _kernel(ref, c, "continuous"))
    X_batch = _t(ref[f"{call}_X_cand"])[idx]
    assert X_batch.shape == (8, 3) and ref["continuous_X"].shape == (8, 3)
    assert np.array_equal(X_batch.numpy(), ref["continuous_X"])


def test_should_reset_prior_equals_the_reference(ref):
    """SOBER/_sober.py:84-123 (when a sampled prior is reset) against `sober_amd.Sober.should_reset_prior` on random
    observation histories; and `next_batch` asks for the caller's `prior_initialiser` instead of dropping
    `recycle_prior` (SOBER/_sober.py:152-155)."""
    import types
    want = ref["reset_verdicts"]
    n_true = 0
    for trial, (n_init, bs, y) in enumerate(MG.reset_histories()):
        model = types.SimpleNamespace(train_targets=y)
        for j, recycle in enumerate((True, False)):
            ra = bool(want[trial, j])
            b = object.__new__(sober_amd.Sober)
            b.n_init, b.n_batches_until_reset, b.pi = n_init, 3, types.SimpleNamespace(model=model)
            rb = bool(b.should_reset_prior(bs, recycle))
            assert ra == rb, (trial, n_init, bs, len(y), recycle)
            n_true += ra
    assert 50 < n_true < 550                                             # (both verdicts occur)

    # a reset that is due and no hook: an error that says so, not a silently recycled prior
    s = object.__new__(sober_amd.Sober)
    s.label, s.n_init, s.n_batches_until_reset, s.prior_initialiser, s.candidate_funnel = "continuous", 2, 3, None, None
    s.pi = types.SimpleNamespace(model=types.SimpleNamespace(train_targets=torch.tensor([5.0, 1, 0, 0, 0, 0, 0, 0])))
    assert s.should_reset_prior(2, True)
    with pytest.raises(NotImplementedError, match="prior_initialiser"):
        s.next_batch(100, 10, 2)
    called = []
    s.prior_initialiser = lambda smp: called.append(smp)
    class _Stop(Exception):
        pass

    def _stop(*a, **k):                                                  # (stop right behind the reset)
        raise _Stop()
    s.candidate_funnel = _stop
    with pytest.raises(_Stop):
        s.next_batch(100, 10, 2)
    assert called == [s]
