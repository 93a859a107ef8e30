"""The oracle against the REFERENCE ITSELF on seeded random cases.  The reference has no tests of its own; the ~25
committed fixtures pin the oracle on the shapes somebody thought of -- this sweep pins it on 64 nobody looked at: kinds x
modes x leftovers of every kind x calc_obj x zero weights x ARD.  The reference's results are stored in
tests/golden/reference_fuzz.npz, written by the same loader that wrote the other fixtures (tests/golden/make_golden.py:
gen_reference_fuzz -- SOBER/_rchq.py:5-270 with SOBER/_kernel.py, _gp.py, _utils.py, no stand-ins above the gpytorch base
kernel, one thread); the inputs are synth(case), their checksums stored beside the results.  Same RNG seed in front of
both calls (the randn draw of torch.svd_lowrank, _rchq.py:34-39).

Bar: identical indices, weights to 1e-12 relative (the two are the same operations in the same order; in practice they
are the same bits on a host whose CPU arithmetic matches the one that recorded the fixture, as for every golden here).  This is what makes the device sweep's verdicts (tests/test_hip_parity.py::test_fuzz_slice_vs_oracle,
tests/tools/fuzz_parity.py) rest on the reference and not on the oracle alone."""
import os
import warnings

import numpy as np
import pytest
import torch

from oracle import sober_oracle as O
from tests.golden.make_golden import fuzz_cases
from tests.golden.synth import synth, build_spec, calc_obj_fn, checksum, SEED_CALL

CASES = fuzz_cases()


@pytest.fixture(scope="module")
def ref():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "reference_fuzz.npz"))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] + "_" + c["kind"] + "_" + c["mode"][:4] for c in CASES])
def test_oracle_equals_reference(ref, case):
    n = case["name"]
    inp = synth(case)
    np.testing.assert_allclose(checksum(inp["X_cand"]), ref[f"{n}_cks_x"], rtol=1e-12)    # the recorded inputs
    if f"{n}_raised" in ref.files:               # the reference itself cannot run this input (e.g. a singular step)
        pytest.skip(f"reference raised {ref[f'{n}_raised']}")
    rec = {k: torch.from_numpy(ref[f"{n}_{k}"]) for k in ("idx", "w", "mu_after")}
    spec = build_spec(case, inp)
    mu = torch.from_numpy(inp["mu0"].copy())
    old = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        torch.manual_seed(SEED_CALL)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            idx, w = O.recombination(torch.from_numpy(inp["X_cand"].copy()), torch.from_numpy(inp["X_nys"].copy()), case["b"],
                                     O.Kernel(spec, case["mode"]), init_weights=mu,
                                     calc_obj=calc_obj_fn if case["calc_obj"] else None)
    finally:
        torch.set_num_threads(old)
    assert torch.equal(idx, rec["idx"]), (idx.tolist(), rec["idx"].tolist())
    assert torch.allclose(w, rec["w"], rtol=1e-12, atol=0.0), float(((w - rec["w"]).abs() / rec["w"].abs()).max())
    assert torch.allclose(mu, rec["mu_after"], rtol=1e-12, atol=0.0)          # Q3: init_weights is mutated in place
