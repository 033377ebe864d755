"""What the device arithmetic tests (tests/test_gpu_device_arith.py) rest on, as far as it holds without a GPU: the numpy
statements of the float-multiply divisions over their stated domains, the integer emulation of rne_div_u32, the caps on
how sensitive the chosen quantiser inputs are to a subtly wrong device step, and that the harness compiles."""
import os

import numpy as np
import pytest

from tests import arith_cases as ac
from tests import arith_harness as ah


def test_divmod_small_statement_over_the_stated_domain():
    """lmc_device.h divmod_small: R 2 .. 30, e < 2^15 (950 272 cases)."""
    e, R = ac.divmod_small_cases()
    q, r, _ = ac.float_divmod(e, R)
    assert np.array_equal(q, e // R) and np.array_equal(r, e % R)


def test_split_divmod_statement_over_the_stated_domain():
    """k_copy_split.h split_divmod: R 4 .. 2048, e < 2048 (4 188 160 cases)."""
    e, R = ac.split_divmod_cases()
    q, r, _ = ac.float_divmod(e, R)
    assert np.array_equal(q, e // R) and np.array_equal(r, e % R)


@pytest.fixture(scope="module")
def counts():
    return {name: ac.sensitivity(ac.QuantDomain(code, np.concatenate([ac.seeded_maxes(code), ac.edge_maxes(code)])))
            for name, code in ac.DTYPES.items()}


@pytest.mark.parametrize("name", list(ac.DTYPES))
def test_quantise_domain_is_sensitive_enough(counts, name):
    """The regular rows of the quantise test (64 seeded in-range maxes + the range's edge patterns, MAX 1 .. 15, every
    finite |x| <= max) must hold at least 50 elements whose symbol a fused multiply-add would change and at least 300
    whose symbol a factor one ulp too large would change; otherwise the GPU test could pass on a wrong device step.
    The maxes of arith_cases.seeded_maxes (default_rng(1)) give bf16 85 / 482 of 32.5 M and fp16 89 / 463 of 34.3 M elements."""
    fused, ulp = counts[name]
    print(f"{name}: single rounding moves {fused} symbols, a one-ulp factor error {ulp}")
    assert fused >= 50 and ulp >= 300


def test_rne_cases_hold_enough_ties_and_the_emulation_is_exact():
    """rne_div_u32 in integers over the GPU test's cases: equal to the rational's RNE everywhere, never more than the two
    corrections the helper has; and the per-T part of the cases alone holds at least 200 exact ties."""
    n, T = ac.rne_cases()
    want, tie = ac.rne_ref(n * ac.CDF_SCALE, T)
    got, need = ac.rne_emulated(n * ac.CDF_SCALE, T)
    assert np.array_equal(got, want)
    assert need.max() <= 2
    n0, T0 = ac.rne_cases(exhaustive_below=0)
    ties = int(np.count_nonzero(ac.rne_ref(n0 * ac.CDF_SCALE, T0)[1]))
    print(f"{len(n)} cases, {int(np.count_nonzero(tie))} ties; without the exhaustive part {len(n0)} cases, {ties} ties; "
          f"corrections needed: up to {int(need.max())}")
    assert ties >= 200


def test_cdf_reference_matches_the_golden_tables(golden_dir):
    """The CDF reference of the GPU test against the tables the reference implementation wrote."""
    z = np.load(os.path.join(golden_dir, "cdf.npz"))
    for T in (1, 7, 16, 128, 236, 250, 256, 768):
        counts, nsym, want, real = ac.golden_cdf_cases(z, T)
        got = ac.cdf_ref(counts, np.full(len(counts), T), nsym) & 0xffff
        assert np.array_equal(got[real], want[real]), T


def test_harness_compiles_with_the_library_flags():
    if not os.path.exists(ah.hipcc()):
        pytest.skip("no hipcc on this box")
    from lmcache_amd import native
    so = ah.build()
    assert os.path.exists(so)
    cmd = ah.command()
    assert cmd[1:1 + len(native.HIPCC_FLAGS)] == native.HIPCC_FLAGS
    # (the library is not loaded here: that needs the HIP runtime, which the GPU tests bring)
