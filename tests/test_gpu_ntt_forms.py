"""GPU: every addressing form of the NTT tile kernel (kernels_ntt.hip: one instantiation per form) at the smallest sizes
that select it, and at the sizes where the dispatcher changes form, byte-equal to the oracle.

  log_n 10      largest single pass (single-pass inverse and LDE)
  log_n 11      smallest two-pass transform: R2 = 32, R1 = 64, a tile narrower than 16
  log_n 12, 13  groups 4+2 and 4+3: the radix-2 remainders beside a radix-16 group
  log_n 16      the hot shape (R = 256, T = 16 in both passes: the constant-shape instantiations)
  log_n 17      first factored pre-scale

Three columns so that the polynomial stride matters, and one.  The quotient stage of a 2^10-row circuit runs the
2^13-point inverse transform from bit-reversed input."""
import numpy as np
import pytest

from conftest import splitmix_field

pytestmark = pytest.mark.gpu

CASES = [(log_n, cols, rate) for log_n in (10, 11, 12, 13) for cols in (3, 1) for rate in (0, 1, 3)]
CASES += [(16, 3, rate) for rate in (0, 1, 3)]
CASES += [(17, cols, 1) for cols in (3, 1)]


@pytest.mark.parametrize("log_n,cols,rate", CASES)
def test_lde_commit_forms_vs_oracle(gpu, oracle, log_n, cols, rate):
    n = 1 << log_n
    vals = splitmix_field(n * cols, seed=1100 + 16 * log_n + 4 * cols + rate).reshape(cols, n)
    cap_h = min(4, log_n + rate)
    for from_coeffs in (False, True):
        co, lo, capo = oracle.lde_commit(vals, rate, cap_h, from_coeffs)
        cg, lg, capg = gpu.lde_commit(vals, rate, cap_h, from_coeffs)
        what = (log_n, cols, rate, from_coeffs)
        assert (cg == co).all(), what
        assert (lg == lo).all(), (what, np.argwhere(lg != lo)[:5])
        assert (capg == capo).all(), what


def test_quotient_stage_inverse_from_bit_reversed_input(gpu, oracle):
    """plonky3-verifier circuit of a 2^3-row Fibonacci STARK: 2^10 rows, quotient evaluated on 2^13 points in leaf order."""
    inp, cfg = gpu.p3_prove_fibonacci(3, 3, 4)
    c = gpu.Circuit.build_p3_verifier(cfg)
    oc = oracle.load_circuit(c.to_blob())
    wires, st, msg = oc.witness(inp, seed=5)
    assert st == 0, msg
    betas, gammas, alphas = splitmix_field(6, seed=31).reshape(3, 2)
    zs = oc.partial_products(wires, betas, gammas)
    qg = c.quotient(wires, zs, betas, gammas, alphas)
    qo = oc.quotient(wires, zs, betas, gammas, alphas)
    assert qg.shape == qo.shape and (qg == qo).all(), np.argwhere(qg != qo)[:5]
    assert qg.any()
