"""CPU: the C ABI's conventions, pinned entry point by entry point (include/p25.h).

- Host-only entry points check their arguments and answer without a device: a null argument is P25_ERR_INVALID_ARG with
  the reason in p25_last_error().
- "buf may be NULL to query the length": the query returns P25_OK and the length, a buffer one element short is
  P25_ERR_INVALID_ARG ("buffer too small") with the length still reported, and an exact-size buffer receives what the
  two-call form returns.
- Device entry points select the device before they look at their arguments: P25_ERR_NO_DEVICE on a box without a GPU
  whatever the arguments, P25_ERR_INVALID_ARG for the same null arguments on a GPU box.  Only arguments the library refuses
  before any launch are passed as NULL here, and no device pointer is ever passed: nothing below can reach a kernel.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import pytest

from conftest import ARTIFACT, P

OK, INVALID_ARG, NO_DEVICE, PARSE, RCCL = 0, 1, 2, 8, 10


def _gpu():
    import torch
    return torch.cuda.is_available()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _out():
    return C.byref(C.c_void_p())


def _fib_trace(log_n):
    rows, a, b = [], 1, 1
    for _ in range(1 << log_n):
        rows.append((a, b, (a + b) % P))
        a, b = b, (a + b) % P
    return np.array(rows, dtype=np.uint64)


@pytest.fixture(scope="module")
def fx(p25):
    lib = p25.lib()
    c = p25.Circuit.build_gadget(0, 0)
    text = open(ARTIFACT, "rb").read()
    inputs, cfg = p25.p3_proof_from_json(text)
    air = p25.Air.fibonacci()
    trace = _fib_trace(3)
    proof = np.zeros(int(c.info.proof_words), dtype=np.uint64)
    f = SimpleNamespace(p25=p25, lib=lib, c=c, h=c._h, text=text, inputs=inputs, cfg=cfg, air=air, air_c=air.to_c(),
                        trace=trace, proof=proof, n=C.c_size_t(0))
    f.ci = p25.binding.CircuitInfo()
    f.u64 = np.zeros(64, dtype=np.uint64)
    f.noncanon = np.zeros(8, dtype=np.uint64)          # one word >= p: refused by the host before any launch
    f.noncanon[5] = P
    f.noncanon12 = np.zeros(12, dtype=np.uint64)
    f.noncanon12[11] = P
    return f


def _last(fx):
    return fx.lib.p25_last_error().decode()


# --------------------------------------------------------------------------------------------------------------------
# host-only entry points: null arguments
# --------------------------------------------------------------------------------------------------------------------
HOST_NULL = {
    "runtime_info": ("out is null", lambda f: f.lib.p25_runtime_info(None)),
    "build_p3_verifier/cfg": ("null argument", lambda f: f.lib.p25_circuit_build_p3_verifier(None, 0, _out())),
    "build_p3_verifier/out": ("null argument", lambda f: f.lib.p25_circuit_build_p3_verifier(C.byref(f.cfg), 0, None)),
    "build_p3_verifier/air": ("unknown AIR", lambda f: f.lib.p25_circuit_build_p3_verifier(C.byref(f.cfg), 7, _out())),
    "build_p3_verifier_air/air": ("null argument",
                                  lambda f: f.lib.p25_circuit_build_p3_verifier_air(C.byref(f.cfg), None, _out())),
    "build_p3_verifier_air/out": ("null argument",
                                  lambda f: f.lib.p25_circuit_build_p3_verifier_air(C.byref(f.cfg), C.byref(f.air_c), None)),
    "build_gadget/out": ("null argument", lambda f: f.lib.p25_circuit_build_gadget(0, 0, None)),
    "build_gate_eval/out": ("null argument", lambda f: f.lib.p25_circuit_build_gate_eval(0, None)),
    "build_gate_eval/kind": ("unknown gate kind", lambda f: f.lib.p25_circuit_build_gate_eval(-1, _out())),
    "circuit_export/c": ("null argument", lambda f: f.lib.p25_circuit_export(None, None, 0, C.byref(f.n))),
    "circuit_export/len": ("null argument", lambda f: f.lib.p25_circuit_export(f.h, None, 0, None)),
    "circuit_import/blob": ("null argument", lambda f: f.lib.p25_circuit_import(None, 0, _out())),
    "circuit_import/out": ("null argument", lambda f: f.lib.p25_circuit_import(_p(f.u64), 8, None)),
    "circuit_from_bytes/bytes": ("null argument",
                                 lambda f: f.lib.p25_circuit_from_bytes(None, 0, None, 0, None, _out())),
    "circuit_from_bytes/targets": ("null argument",
                                   lambda f: f.lib.p25_circuit_from_bytes(_p(f.u64), 8, None, 3, None, _out())),
    "circuit_input_targets/c": ("null argument", lambda f: f.lib.p25_circuit_input_targets(None, None, 0, C.byref(f.n))),
    "circuit_input_targets/n": ("null argument", lambda f: f.lib.p25_circuit_input_targets(f.h, None, 0, None)),
    "circuit_info/c": ("null argument", lambda f: f.lib.p25_circuit_info(None, C.byref(f.ci))),
    "circuit_info/out": ("null argument", lambda f: f.lib.p25_circuit_info(f.h, None)),
    "gate_counts/c": ("null argument", lambda f: f.lib.p25_circuit_gate_counts(None, _p(f.u64), 64, None, 0)),
    "gate_counts/counts": ("null argument", lambda f: f.lib.p25_circuit_gate_counts(f.h, None, 64, None, 0)),
    "set_streams/c": ("null argument", lambda f: f.lib.p25_circuit_set_streams(None, 4)),
    "set_streams/n": ("n_streams must be in 1..32", lambda f: f.lib.p25_circuit_set_streams(f.h, 0)),
    "p3_proof_from_json/json": ("null argument",
                                lambda f: f.lib.p25_p3_proof_from_json(None, 0, None, 0, C.byref(f.n), None)),
    "p3_proof_from_json/n": ("null argument",
                             lambda f: f.lib.p25_p3_proof_from_json(f.text, len(f.text), None, 0, None, None)),
    "p3_prove_fibonacci/n": ("null argument", lambda f: f.lib.p25_p3_prove_fibonacci(3, 3, 4, 0, 1, None, 0, None, None)),
    "p3_prove_fibonacci/params": ("bad parameters",
                                  lambda f: f.lib.p25_p3_prove_fibonacci(0, 3, 4, 0, 1, None, 0, C.byref(f.n), None)),
    "p3_prove_air_ex/air": ("null argument", lambda f: f.lib.p25_p3_prove_air_ex(None, None, 3, 1, 3, 4, 0, 1, None, 0,
                                                                                 C.byref(f.n), None)),
    "p3_prove_air_ex/n": ("null argument", lambda f: f.lib.p25_p3_prove_air_ex(C.byref(f.air_c), None, 3, 1, 3, 4, 0, 1,
                                                                               None, 0, None, None)),
    "p3_prove_air_ex/trace": ("null trace", lambda f: f.lib.p25_p3_prove_air_ex(C.byref(f.air_c), None, 3, 1, 3, 4, 0, 1,
                                                                                _p(f.u64), 64, C.byref(f.n), None)),
    "p3_prove_air/air": ("null argument", lambda f: f.lib.p25_p3_prove_air(None, None, 3, 3, 4, 0, 1, None, 0,
                                                                           C.byref(f.n), None)),
    "p3_inputs_to_json/inputs": ("null argument", lambda f: f.lib.p25_p3_inputs_to_json(None, 0, C.byref(f.cfg), None, 0,
                                                                                        C.byref(f.n))),
    "p3_inputs_to_json/cfg": ("null argument", lambda f: f.lib.p25_p3_inputs_to_json(_p(f.inputs), f.inputs.size, None,
                                                                                     None, 0, C.byref(f.n))),
    "p3_inputs_to_json/len": ("null argument", lambda f: f.lib.p25_p3_inputs_to_json(_p(f.inputs), f.inputs.size,
                                                                                     C.byref(f.cfg), None, 0, None)),
    "proof_to_json/c": ("null argument", lambda f: f.lib.p25_proof_to_json(None, _p(f.proof), None, 0, C.byref(f.n))),
    "proof_to_json/proof": ("null argument", lambda f: f.lib.p25_proof_to_json(f.h, None, None, 0, C.byref(f.n))),
    "proof_to_json/len": ("null argument", lambda f: f.lib.p25_proof_to_json(f.h, _p(f.proof), None, 0, None)),
    "proof_to_bytes/c": ("null argument", lambda f: f.lib.p25_proof_to_bytes(None, _p(f.proof), None, 0, C.byref(f.n))),
    "proof_to_bytes/proof": ("null argument", lambda f: f.lib.p25_proof_to_bytes(f.h, None, None, 0, C.byref(f.n))),
    "proof_to_bytes/len": ("null argument", lambda f: f.lib.p25_proof_to_bytes(f.h, _p(f.proof), None, 0, None)),
    "proof_from_bytes/c": ("null argument",
                           lambda f: f.lib.p25_proof_from_bytes(None, _p(f.u64), 8, _p(f.proof), f.proof.size)),
    "proof_from_bytes/bytes": ("null argument",
                               lambda f: f.lib.p25_proof_from_bytes(f.h, None, 8, _p(f.proof), f.proof.size)),
    "proof_from_bytes/out": ("null argument", lambda f: f.lib.p25_proof_from_bytes(f.h, _p(f.u64), 8, None, f.proof.size)),
}


@pytest.mark.parametrize("case", sorted(HOST_NULL))
def test_host_entry_point_refuses_null_argument(fx, case):
    text, call = HOST_NULL[case]
    assert call(fx) == INVALID_ARG
    assert text in _last(fx)


def test_size_functions_return_zero_for_a_bad_shape(fx):
    lib = fx.lib
    assert lib.p25_merkle_tree_words(8, 2) > 0
    assert lib.p25_merkle_tree_words(12, 0) == 0 and lib.p25_merkle_tree_words(8, 4) == 0
    ar = np.array([1, 1], dtype=np.int32)
    assert lib.p25_fri_prove_words(6, 1, 2, _p(ar), 2, 3) > 0
    assert lib.p25_fri_prove_words(6, 1, 9, None, 0, 3) == 0 and lib.p25_fri_prove_words(6, 1, 2, None, 1, 3) == 0


# --------------------------------------------------------------------------------------------------------------------
# host-only entry points: "buf may be NULL to query the length"
# --------------------------------------------------------------------------------------------------------------------
# name -> (element dtype, call(f, buf, cap, len_ref), the two-call result through the binding)
SIZED = {
    "circuit_export": (np.uint8, lambda f, b, cap, n: f.lib.p25_circuit_export(f.h, b, cap, n),
                       lambda f: np.frombuffer(f.c.to_blob(), dtype=np.uint8)),
    "circuit_input_targets": (np.uint32, lambda f, b, cap, n: f.lib.p25_circuit_input_targets(f.h, b, cap, n),
                              lambda f: f.c.input_target_indices()),
    "p3_proof_from_json": (np.uint64, lambda f, b, cap, n: f.lib.p25_p3_proof_from_json(f.text, len(f.text), b, cap, n, None),
                           lambda f: f.p25.p3_proof_from_json(f.text)[0]),
    "p3_prove_fibonacci": (np.uint64, lambda f, b, cap, n: f.lib.p25_p3_prove_fibonacci(3, 3, 4, 0, 1, b, cap, n, None),
                           lambda f: f.p25.p3_prove_fibonacci(3, 3, 4, threads=1)[0]),
    "p3_prove_air_ex": (np.uint64, lambda f, b, cap, n: f.lib.p25_p3_prove_air_ex(C.byref(f.air_c), _p(f.trace), 3, 1, 3, 4,
                                                                                  0, 1, b, cap, n, None),
                        lambda f: f.p25.p3_prove_air(f.air, f.trace, num_queries=3, pow_bits=4, threads=1)[0]),
    "p3_inputs_to_json": (np.uint8, lambda f, b, cap, n: f.lib.p25_p3_inputs_to_json(_p(f.inputs), f.inputs.size,
                                                                                     C.byref(f.cfg), b, cap, n),
                          lambda f: np.frombuffer(f.p25.p3_inputs_to_json(f.inputs, f.cfg).encode(), dtype=np.uint8)),
    "proof_to_json": (np.uint8, lambda f, b, cap, n: f.lib.p25_proof_to_json(f.h, _p(f.proof), b, cap, n),
                      lambda f: np.frombuffer(f.c.proof_to_json(f.proof).encode(), dtype=np.uint8)),
    "proof_to_bytes": (np.uint8, lambda f, b, cap, n: f.lib.p25_proof_to_bytes(f.h, _p(f.proof), b, cap, n),
                       lambda f: np.frombuffer(f.c.proof_to_bytes(f.proof), dtype=np.uint8)),
}


@pytest.mark.parametrize("case", sorted(SIZED))
def test_size_query_protocol(fx, case):
    dtype, call, two_call = SIZED[case]
    want = two_call(fx)
    assert want.size > 0
    n = C.c_size_t(0)
    assert call(fx, None, 0, C.byref(n)) == OK and n.value == want.size
    buf = np.zeros(want.size, dtype=dtype)
    n.value = 0
    assert call(fx, _p(buf), want.size - 1, C.byref(n)) == INVALID_ARG
    assert "buffer too small" in _last(fx) and n.value == want.size
    n.value = 0
    assert call(fx, _p(buf), want.size, C.byref(n)) == OK and n.value == want.size
    assert buf.tobytes() == want.astype(dtype).tobytes()


def test_capacity_only_entry_points(fx):
    lib = fx.lib
    n_gates = len(fx.c.gate_counts())
    counts = np.zeros(n_gates, dtype=np.uint64)
    assert lib.p25_circuit_gate_counts(fx.h, _p(counts), n_gates - 1, None, 0) == INVALID_ARG
    assert "buffer too small" in _last(fx)
    assert lib.p25_circuit_gate_counts(fx.h, _p(counts), n_gates, None, 0) == OK
    assert counts.tolist() == list(fx.c.gate_counts().values())
    data = np.frombuffer(fx.c.proof_to_bytes(fx.proof), dtype=np.uint8).copy()
    out = np.ones(fx.proof.size, dtype=np.uint64)
    assert lib.p25_proof_from_bytes(fx.h, _p(data), data.size, _p(out), out.size - 1) == INVALID_ARG
    assert "buffer too small" in _last(fx)
    assert lib.p25_proof_from_bytes(fx.h, _p(data), data.size, _p(out), out.size) == OK
    assert (out == fx.proof).all()


def test_p3_proof_from_json_reports_parse_errors_as_parse(fx):
    lib, n = fx.lib, C.c_size_t(0)
    bad = fx.text[: len(fx.text) // 2]
    assert lib.p25_p3_proof_from_json(bad, len(bad), None, 0, C.byref(n), None) == PARSE
    assert _last(fx).startswith("p3 proof JSON")
    # the remapping is for the reader's own messages only: argument and capacity errors stay INVALID_ARG
    assert lib.p25_p3_proof_from_json(None, 0, None, 0, C.byref(n), None) == INVALID_ARG
    small = np.zeros(4, dtype=np.uint64)
    assert lib.p25_p3_proof_from_json(fx.text, len(fx.text), _p(small), 4, C.byref(n), None) == INVALID_ARG


def test_fibonacci_size_query_reports_the_shape(fx):
    """The size query answers without proving, with the shape the proof will have (proof_of_work_bits included)."""
    n, cfg_q, cfg = C.c_size_t(0), fx.p25.P3Config(), fx.p25.P3Config()
    assert fx.lib.p25_p3_prove_fibonacci(3, 3, 4, 0, 1, None, 0, C.byref(n), C.byref(cfg_q)) == OK
    buf = np.zeros(n.value, dtype=np.uint64)
    assert fx.lib.p25_p3_prove_fibonacci(3, 3, 4, 0, 1, _p(buf), buf.size, C.byref(n), C.byref(cfg)) == OK
    assert bytes(cfg_q) == bytes(cfg)
    assert (cfg.log_trace_height, cfg.num_queries, cfg.proof_of_work_bits, cfg.degree_bits) == (3, 3, 4, 3)


# --------------------------------------------------------------------------------------------------------------------
# device entry points: the device comes first
# --------------------------------------------------------------------------------------------------------------------
def _cnt():
    return (C.c_size_t * 1)(0)


# name -> (reason on a GPU box, or None where NULL is not refused before a launch: never called there; call)
DEVICE_NULL = {
    "shader_clock_hz": ("hz_out is null", lambda f: f.lib.p25_shader_clock_hz(None)),
    "poseidon_permute": ("states is null", lambda f: f.lib.p25_poseidon_permute(None, 1)),
    "poseidon2_permute": ("states is null", lambda f: f.lib.p25_poseidon2_permute(None, 1)),
    "poseidon2_permute/canonical": ("non-canonical field element",
                                    lambda f: f.lib.p25_poseidon2_permute(_p(f.noncanon12), 1)),
    "poseidon_permute_dev": (None, lambda f: f.lib.p25_poseidon_permute_dev(None, 0, None)),
    "merkle_commit": ("bad shape", lambda f: f.lib.p25_merkle_commit(None, 8, 1, 0, None, None)),
    "merkle_commit/canonical": ("non-canonical field element",
                                lambda f: f.lib.p25_merkle_commit(_p(f.noncanon), 8, 1, 0, _p(f.u64), None)),
    "merkle_commit_dev": ("bad shape", lambda f: f.lib.p25_merkle_commit_dev(None, 8, 8, 1, 0, None, None)),
    "merkle_commit_dev/stride": ("bad shape", lambda f: f.lib.p25_merkle_commit_dev(None, 7, 8, 1, 0, None, None)),
    "merkle_commit_dev/width": ("width above 2^20",
                                lambda f: f.lib.p25_merkle_commit_dev(None, 8, 8, (1 << 20) + 1, 0, None, None)),
    "lde_commit": ("bad shape", lambda f: f.lib.p25_lde_commit(None, 3, 1, 0, 1, 0, None, None, None)),
    "lde_commit/canonical": ("non-canonical field element",
                             lambda f: f.lib.p25_lde_commit(_p(f.noncanon), 3, 1, 0, 1, 0, None, None, _p(f.u64))),
    "lde_commit/canonical_coeffs": ("non-canonical field element",
                                    lambda f: f.lib.p25_lde_commit(_p(f.noncanon), 3, 1, 1, 1, 0, None, None, _p(f.u64))),
    "lde_commit_dev": ("bad shape", lambda f: f.lib.p25_lde_commit_dev(None, 3, 1, 0, 1, 0, None, None, None, None, None)),
    "lde_commit_dev/cap": ("cap_height above log_n + rate_bits",
                           lambda f: f.lib.p25_lde_commit_dev(None, 2, 1, 0, 1, 4, None, None, None, None, None)),
    "lde_commit/cap": ("bad shape", lambda f: f.lib.p25_lde_commit(_p(f.u64), 2, 1, 0, 1, 4, None, None, _p(f.u64))),
    "circuit_to_bytes": ("null argument", lambda f: f.lib.p25_circuit_to_bytes(f.h, None, None)),
    "circuit_digest/c": ("null argument", lambda f: f.lib.p25_circuit_digest(None, _p(f.u64), None)),
    "circuit_digest/digest": ("null argument", lambda f: f.lib.p25_circuit_digest(f.h, None, None)),
    "build_recursive_verifier": ("null argument",
                                 lambda f: f.lib.p25_circuit_build_recursive_verifier(f.h, None, None, 1, None)),
    "build_aggregator": ("null argument", lambda f: f.lib.p25_circuit_build_aggregator(None, None, None, 2, _out())),
    "prove_batch": ("null argument", lambda f: f.lib.p25_prove_batch(f.h, None, 1, None, None, 1, None, None)),
    "prove_batch_filler": ("null argument", lambda f: f.lib.p25_prove_batch_filler(f.h, None, 1, None, None, 1, None)),
    "prove_batch_dev": ("null argument", lambda f: f.lib.p25_prove_batch_dev(f.h, None, 1, None, None, 1, None, None)),
    "prove_batch_dev_windows": ("null argument", lambda f: f.lib.p25_prove_batch_dev_windows(f.h, None, 1, 0, 1, None, None,
                                                                                             1, None)),
    "circuit_sync": ("null argument", lambda f: f.lib.p25_circuit_sync(None)),
    "circuit_stream_join": ("null argument", lambda f: f.lib.p25_circuit_stream_join(None, None)),
    "circuit_wait_stream": ("null argument", lambda f: f.lib.p25_circuit_wait_stream(None, None)),
    "circuit_mark": ("null argument", lambda f: f.lib.p25_circuit_mark(None, 0)),
    "circuit_stream_wait_mark": ("null argument", lambda f: f.lib.p25_circuit_stream_wait_mark(None, 0, None)),
    "circuit_wait_mark/null": ("null argument", lambda f: f.lib.p25_circuit_wait_mark(f.h, None, 0)),
    "circuit_wait_mark/self": ("already in order", lambda f: f.lib.p25_circuit_wait_mark(f.h, f.h, 0)),
    "circuit_kernel_stats": ("null argument", lambda f: f.lib.p25_circuit_kernel_stats(None, 1, 0, None, None)),
    "witness": ("null argument", lambda f: f.lib.p25_witness(f.h, None, 0, None, None)),
    "transcript": ("null argument", lambda f: f.lib.p25_transcript(None, None, None, 1, None)),
    "transcript/canonical": ("non-canonical field element",
                             lambda f: f.lib.p25_transcript(_p(f.noncanon), _p(np.array([8], dtype=np.uint32)),
                                                            _p(np.array([1], dtype=np.uint32)), 1, _p(f.u64))),
    "partial_products": ("null argument", lambda f: f.lib.p25_partial_products(f.h, None, None, None, None)),
    "quotient": ("null argument", lambda f: f.lib.p25_quotient(f.h, None, None, None, None, None, None)),
    "eval_polys": ("null argument", lambda f: f.lib.p25_eval_polys(None, 1, 3, None, 1, None)),
    "fri_prove": ("null argument", lambda f: f.lib.p25_fri_prove(None, 6, 1, 2, None, 0, 0, 3, None, 0, None, 0, None)),
}


@pytest.mark.parametrize("case", sorted(DEVICE_NULL))
def test_device_entry_point_checks_the_device_first(fx, case):
    text, call = DEVICE_NULL[case]
    if not _gpu():
        assert call(fx) == NO_DEVICE
        assert "no CPU fallback" in _last(fx)
    elif text is None:
        pytest.skip("NULL is not refused before a launch here")
    else:
        assert call(fx) == INVALID_ARG
        assert text in _last(fx)


COMM_NULL = {
    "comm_sync": lambda f: f.lib.p25_comm_sync(None),
    "comm_barrier": lambda f: f.lib.p25_comm_barrier(None),
    "comm_max_f64": lambda f: f.lib.p25_comm_max_f64(None, None),
    "comm_unique_id": lambda f: f.lib.p25_comm_unique_id(None),
    "comm_init": lambda f: f.lib.p25_comm_init(None, 0, 1, _out()),
    "gather_proofs": lambda f: f.lib.p25_gather_proofs(None, None, -1, None, 1, None, _cnt(), 0, None, None),
}


@pytest.mark.parametrize("case", sorted(COMM_NULL))
def test_comm_entry_point_checks_the_device_then_rccl_first(fx, case):
    st = COMM_NULL[case](fx)
    if not _gpu():
        assert st == NO_DEVICE
    elif st == RCCL:
        assert "librccl" in _last(fx)
    else:
        assert st == INVALID_ARG and "null" in _last(fx)


def test_fri_prove_capacity_check(fx):
    """p25_fri_prove refuses a short output buffer before it runs anything (device guard first)."""
    ar = np.array([1, 1], dtype=np.int32)
    words = fx.lib.p25_fri_prove_words(6, 1, 2, _p(ar), 2, 3)
    coeffs = np.zeros((2, 64), dtype=np.uint64)
    out = np.zeros(words, dtype=np.uint64)
    st = C.c_int32(0)
    s = fx.lib.p25_fri_prove(_p(coeffs), 6, 1, 2, _p(ar), 2, 0, 3, None, 0, _p(out), words - 1, C.byref(st))
    if not _gpu():
        assert s == NO_DEVICE
    else:
        assert s == INVALID_ARG and "buffer too small" in _last(fx)


def test_build_recursive_guard_follows_digest(fx):
    """With digest4 / cs_cap given the recursive builders are host-only; without them they need the device for the inner
    circuit's digest."""
    lib, h = fx.lib, fx.h
    dg = np.zeros(4, dtype=np.uint64)
    cap = np.zeros(4 << 10, dtype=np.uint64)
    for fn in (lib.p25_circuit_build_recursive_verifier, lib.p25_circuit_build_aggregator):
        assert fn(h, _p(dg), None, 2, _out()) == INVALID_ARG and "pass both" in _last(fx)
        assert fn(None, _p(dg), _p(cap), 2, _out()) == INVALID_ARG and "null argument" in _last(fx)
        assert fn(h, _p(dg), _p(cap), 2, None) == INVALID_ARG and "null argument" in _last(fx)
        bad = dg.copy()
        bad[1] = P
        assert fn(h, _p(bad), _p(cap), 2, _out()) == INVALID_ARG and "non-canonical digest word" in _last(fx)
        # digest4 alone picks the guard: without it the device comes first, whatever else is wrong
        for args, text in (((None, None, None), "null argument"), ((h, None, _p(cap)), "pass both")):
            st = fn(*args, 2, _out())
            if not _gpu():
                assert st == NO_DEVICE and "no CPU fallback" in _last(fx)
            else:
                assert st == INVALID_ARG and text in _last(fx)
    out = C.c_void_p()
    assert lib.p25_circuit_build_recursive_verifier(h, _p(dg), _p(cap), 1, C.byref(out)) == OK and out.value
    lib.p25_circuit_destroy(out)
