"""GPU: the plonky3 prover on the device (P3Prover: p25_p3_prove_batch, p25_p3_prove_batch_dev) against the host prover.

The yardstick is p3_prove_air / p3_prove_fibonacci (which reproduce the reference's artifacts/proof_fibonacci.json bit for
bit, tests/test_p3_prover.py): for the same arguments the device prover must return THE SAME WORDS.  Field arithmetic is
exact, so every comparison is np.array_equal; there is no tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import air_cases
from conftest import P
from device_buffers import Banded, Banded32, strided_rows

pytestmark = pytest.mark.gpu

OK, INVALID_ARG = 0, 1


def _host(gpu, air, trace, q, pow_bits, log_blowup=1, pow_start=0):
    return gpu.p3_prove_air(air, trace, num_queries=q, pow_bits=pow_bits, pow_start=pow_start, log_blowup=log_blowup)[0]


def _check_one(gpu, air, trace, q, pow_bits, log_blowup=1):
    log_n = int(trace.shape[0]).bit_length() - 1
    pr = gpu.P3Prover(air, log_n, log_blowup, q, pow_bits)
    got, st = pr.prove(trace)
    assert st.tolist() == [OK]
    want = _host(gpu, air, trace, q, pow_bits, log_blowup)
    assert got.shape == (1, want.size)
    bad = np.nonzero(got[0] != want)[0]
    assert bad.size == 0, f"{bad.size} of {want.size} words differ, first at {bad[:8].tolist()}"
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 1. the reference's artifact
# ---------------------------------------------------------------------------------------------------------------------
def test_reproduces_the_references_artifact(gpu, fib_inputs):
    pr = gpu.P3Prover(gpu.Air.fibonacci(), 6, 1, 100, 16)
    got, st = pr.prove(air_cases.fib_trace(6), pow_starts=[0])
    assert st.tolist() == [OK]
    assert pr.num_inputs == fib_inputs.size == 15751
    assert np.array_equal(got[0], fib_inputs)


# ---------------------------------------------------------------------------------------------------------------------
# 2. sizes: degenerate trees (1, 2), one- and two-pass transforms (10 | 11), FRI all in the workgroup tail (<= 9), one
#    round (10), two (11) and four (13) rounds of separate launches in front of it
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("log_n,q,pow_bits", [(1, 1, 0), (2, 4, 8), (3, 100, 16), (6, 4, 8), (9, 1, 0), (10, 100, 16),
                                              (11, 4, 8), (13, 100, 16)])
def test_fibonacci_sizes(gpu, log_n, q, pow_bits):
    _check_one(gpu, gpu.Air.fibonacci(), air_cases.fib_trace(log_n), q, pow_bits)
    if log_n == 6:     # the Fibonacci entry point of the host is the same yardstick
        want, _cfg = gpu.p3_prove_fibonacci(log_n, q, pow_bits)
        got, _st = gpu.P3Prover(gpu.Air.fibonacci(), log_n, 1, q, pow_bits).prove(air_cases.fib_trace(log_n))
        assert np.array_equal(got[0], want)


# ---------------------------------------------------------------------------------------------------------------------
# 3. widths and degrees
# ---------------------------------------------------------------------------------------------------------------------
def _sextic(p25, a, c, x0):
    """Degree 6 in an ALWAYS constraint (eight quotient chunks): y = x^6 + a on every row, next x = y + c x, first row x0."""
    air = p25.Air(2)
    x, y = air.local(0), air.local(1)
    x2 = air.mul(x, x)
    x6 = air.mul(air.mul(x2, x2), x2)
    air.assert_zero(air.sub(air.add(x6, air.const(a)), y))
    air.when_transition(air.sub(air.next(0), air.add(y, air.mul(air.const(c), x))))
    air.when_first_row(air.sub(x, air.const(x0)))
    return air


def _sextic_trace(a, c, x, log_n):
    t = np.zeros((1 << log_n, 2), dtype=np.uint64)
    for i in range(1 << log_n):
        y = (pow(x, 6, P) + a) % P
        t[i] = (x, y)
        x = (y + c * x) % P
    return t


def _air_case(p25, name):
    """(air, trace, log_blowup)"""
    if name == "tribonacci":
        return air_cases.tribonacci(p25), air_cases.tribonacci_trace(4), 1
    if name == "squares":
        return air_cases.squares(p25), air_cases.squares_trace(5), 1
    if name.startswith("random_recurrence"):
        w = int(name.split("/")[1])
        air, coef = air_cases.random_recurrence(p25, 40 + w, w)
        return air, air_cases.random_recurrence_trace(coef, 4), 1
    if name == "quadratic_pair":
        air, par = air_cases.quadratic_pair(p25, 5)
        return air, air_cases.quadratic_pair_trace(par, 4), 1
    if name == "cubic":
        return air_cases.cubic(p25), air_cases.cubic_trace(5), 1
    if name == "cubic_transition":
        return air_cases.cubic_transition(p25), air_cases.cubic_transition_trace(4), 1
    if name.startswith("quartic_map"):
        air, par = air_cases.quartic_map(p25, 6)
        return air, air_cases.quartic_map_trace(par, 4), int(name.split("/")[1])
    if name == "quintic_selector":
        air, par = air_cases.quintic_selector(p25, 8)
        return air, air_cases.quintic_selector_trace(par, 4), 2
    if name == "sextic":
        return _sextic(p25, 11, 5, 3), _sextic_trace(11, 5, 3, 4), 3
    assert name == "fibonacci/blowup4"
    return p25.Air.fibonacci(), air_cases.fib_trace(5), 4


@pytest.mark.parametrize("name", ["tribonacci", "squares", "random_recurrence/2", "random_recurrence/5", "random_recurrence/9",
                                  "quadratic_pair", "cubic", "cubic_transition", "quartic_map/2", "quartic_map/3",
                                  "quintic_selector", "sextic", "fibonacci/blowup4"])
def test_widths_and_degrees(gpu, name):
    air, trace, log_blowup = _air_case(gpu, name)
    _check_one(gpu, air, trace, 5, 6, log_blowup)


# ---------------------------------------------------------------------------------------------------------------------
# 4. batch and pow_starts
# ---------------------------------------------------------------------------------------------------------------------
POW_STARTS = [0, 1, 1 << 20, 1 << 40, P - (1 << 20)]


@pytest.fixture(scope="module")
def squares5(gpu):
    """Five `squares` traces and the host's proof of each from its own pow_start: computed once, never changed."""
    air = air_cases.squares(gpu)
    traces = np.stack([air_cases.squares_trace(5, seed=s) for s in range(1, 6)])
    want = np.stack([_host(gpu, air, traces[i], 6, 10, pow_start=POW_STARTS[i]) for i in range(5)])
    want.setflags(write=False)
    return air, traces, want


def test_batch_with_pow_starts(gpu, squares5):
    air, traces, want = squares5
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    got, st = pr.prove(traces, pow_starts=POW_STARTS)
    assert st.tolist() == [OK] * 5
    for i in range(5):
        assert np.array_equal(got[i], want[i]), f"proof {i}"
        for j in range(i):
            assert not np.array_equal(got[i], got[j])
    # the witness found is the smallest one at or above its start
    w_off = pr.num_inputs - 1 - 6 * (3 + 2 + 8 * 6)
    assert all(int(got[i, w_off]) >= POW_STARTS[i] for i in range(5))
    again, st2 = pr.prove(traces, pow_starts=POW_STARTS)
    assert st2.tolist() == [OK] * 5 and np.array_equal(again, got)


def test_grouping_changes_no_word(gpu, squares5):
    """40 proofs under a scratch budget that holds about 8 of them (and under one that holds a single proof): group
    boundaries fall inside the batch, every row is the one the five-proof call gave.  Then 41: a group of eight does not
    divide it, the last group is short."""
    air, traces, want = squares5
    for n in (40, 41):
        pick = np.arange(n) % 5
        for budget in (200_000, 1):
            pr = gpu.P3Prover(air, 5, 1, 6, 10)
            pr.set_scratch_budget(budget)
            got, st = pr.prove(traces[pick], pow_starts=np.array(POW_STARTS, dtype=np.uint64)[pick])
            assert st.tolist() == [OK] * n
            assert np.array_equal(got, want[pick])
            pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 5. a trace that violates the AIR fails its own proof only
# ---------------------------------------------------------------------------------------------------------------------
def test_rejected_trace(gpu, squares5):
    air, traces, want = squares5
    bad = traces[:3].copy()
    bad[1, 7, 1] = (int(bad[1, 7, 1]) + 1) % P
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    got, st = pr.prove(bad, pow_starts=POW_STARTS[:3])
    assert st.tolist() == [OK, INVALID_ARG, OK]
    assert not got[1].any()
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[2], want[2])
    with pytest.raises(gpu.P25Error) as e:      # the host's verdict for that trace alone
        _host(gpu, air, bad[1], 6, 10, pow_start=1)
    assert e.value.status == INVALID_ARG


# ---------------------------------------------------------------------------------------------------------------------
# 6. where it reads and writes
# ---------------------------------------------------------------------------------------------------------------------
ODD = 4097


def _dev_run(pr, traces, pow_starts, t_stride, i_stride, stream=None, occupy=None):
    """prove_dev on guard-banded buffers; returns (inputs[n][num_inputs], statuses) after checking every band."""
    import torch
    n, tw, ni = traces.shape[0], traces[0].size, pr.num_inputs
    d_tr, d_ps = Banded(n * t_stride, before=ODD), Banded(n, before=ODD)
    d_in, d_st = Banded(n * i_stride, before=ODD), Banded32(n, before=ODD)
    t_data, t_pad = strided_rows(n, tw, t_stride)
    interior = d_tr.get()
    interior[t_data] = traces.reshape(n, tw).ravel()
    d_ps.set(np.asarray(pow_starts, dtype=np.uint64))
    if stream is None:
        d_tr.set(interior)
        torch.cuda.synchronize()
    else:
        d_tr.set_async(interior, stream, before_enqueue=occupy)
    pr.prove_dev(d_tr.ptr, t_stride, n, d_ps.ptr, d_in.ptr, i_stride, d_st.ptr, stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    else:
        pr.sync()
    d_tr.assert_unchanged()
    d_ps.assert_unchanged()
    d_in.assert_bands_intact()
    d_st.assert_bands_intact()
    i_data, i_pad = strided_rows(n, ni, i_stride)
    d_in.assert_untouched(i_pad)
    return d_in.get()[i_data].reshape(n, ni), d_st.get()


def test_strides_and_guard_bands(gpu, squares5):
    air, traces, want = squares5
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    got, st = _dev_run(pr, traces, POW_STARTS, traces[0].size + 5, pr.num_inputs + 3)
    assert st.tolist() == [OK] * 5
    assert np.array_equal(got, want)
    packed, st = _dev_run(pr, traces, POW_STARTS, traces[0].size, pr.num_inputs)
    assert st.tolist() == [OK] * 5 and np.array_equal(packed, got)


# ---------------------------------------------------------------------------------------------------------------------
# 7. the caller's stream
# ---------------------------------------------------------------------------------------------------------------------
def test_runs_on_the_callers_stream(gpu, squares5):
    """The traces arrive ON the side stream, as a copy queued behind milliseconds of other work; until the stream gets
    there the trace buffer holds sentinels (words >= p).  A launch or copy of the prover anywhere else starts at once and
    reads them, or reads what its predecessor has not written: the proofs would differ.  Nothing lands early; the result
    is read after stream.synchronize() only."""
    import torch
    air, traces, want = squares5
    dev = torch.device("cuda", 0)
    lib = gpu.lib()
    n, w = 1 << 19, 135
    cols = torch.randint(0, 1 << 62, (w * n,), dtype=torch.int64, device=dev)
    tree = torch.zeros(int(lib.p25_merkle_tree_words(n, 4)), dtype=torch.int64, device=dev)
    side = torch.cuda.Stream(device=dev)
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    warm, st = pr.prove(traces[:1], pow_starts=POW_STARTS[:1])     # tables and scratch exist before the timed order matters
    assert st.tolist() == [OK]
    torch.cuda.synchronize()

    def occupy():
        assert lib.p25_merkle_commit_dev(C.c_void_p(cols.data_ptr()), n, n, w, 4, C.c_void_p(tree.data_ptr()),
                                         C.c_void_p(side.cuda_stream)) == 0

    got, st = _dev_run(pr, traces, POW_STARTS, traces[0].size + 5, pr.num_inputs + 3, stream=side, occupy=occupy)
    assert st.tolist() == [OK] * 5
    assert np.array_equal(got, want)
    torch.cuda.synchronize()


def _plain_dev_call(pr, traces, pow_starts, stream):
    """prove_dev on plain device tensors, enqueued on `stream` and NOT waited for; returns the tensors that keep the
    buffers alive: (traces, starts, inputs, statuses)."""
    import torch
    dev = torch.device("cuda", 0)
    n = traces.shape[0]
    d_tr = torch.from_numpy(traces.reshape(n, -1).view(np.int64).copy()).to(dev)
    d_ps = torch.from_numpy(np.asarray(pow_starts, dtype=np.uint64).view(np.int64).copy()).to(dev)
    d_in = torch.zeros((n, pr.num_inputs), dtype=torch.int64, device=dev)
    d_st = torch.full((n,), 77, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    pr.prove_dev(d_tr.data_ptr(), traces[0].size, n, d_ps.data_ptr(), d_in.data_ptr(), pr.num_inputs, d_st.data_ptr(),
                 stream.cuda_stream)
    return d_tr, d_ps, d_in, d_st


def test_two_streams_share_the_scratch_in_turn(gpu, squares5):
    """Two calls on two streams, the second enqueued while the first is in flight: both work in the handle's one scratch
    region, so the second must wait for the first ON THE DEVICE.  Different traces per call: a call that ran over the
    other's trees or transcripts gives other words or a failure status."""
    import torch
    air, traces, want = squares5
    dev = torch.device("cuda", 0)
    pick_a, pick_b = np.arange(20) % 5, (np.arange(20) * 3 + 2) % 5
    starts = np.array(POW_STARTS, dtype=np.uint64)
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    s1, s2 = torch.cuda.Stream(device=dev), torch.cuda.Stream(device=dev)
    a = _plain_dev_call(pr, traces[pick_a], starts[pick_a], s1)
    b = _plain_dev_call(pr, traces[pick_b], starts[pick_b], s2)
    c = _plain_dev_call(pr, traces[pick_a[::-1]], starts[pick_a[::-1]], s1)
    pr.sync()       # the latest record covers every call before it
    for (d_tr, d_ps, d_in, d_st), pick in ((a, pick_a), (b, pick_b), (c, pick_a[::-1])):
        assert d_st.cpu().numpy().tolist() == [OK] * 20
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64), want[pick])
    torch.cuda.synchronize()
    pr.close()


def test_host_form_behind_a_device_call_in_flight(gpu, squares5):
    """The host form runs on the handle's own stream; an earlier device call on the caller's stream may still be running
    in the same scratch.  Both equal the host prover's rows, and so does a device call enqueued after the host form."""
    import torch
    air, traces, want = squares5
    dev = torch.device("cuda", 0)
    pick_a, pick_b = np.arange(20) % 5, (np.arange(20) * 2 + 1) % 5
    starts = np.array(POW_STARTS, dtype=np.uint64)
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    side = torch.cuda.Stream(device=dev)
    a = _plain_dev_call(pr, traces[pick_a], starts[pick_a], side)
    got_b, st_b = pr.prove(traces[pick_b], pow_starts=starts[pick_b])
    c = _plain_dev_call(pr, traces[pick_b], starts[pick_b], side)
    assert st_b.tolist() == [OK] * 20 and np.array_equal(got_b, want[pick_b])
    side.synchronize()
    for (d_tr, d_ps, d_in, d_st), pick in ((a, pick_a), (c, pick_b)):
        assert d_st.cpu().numpy().tolist() == [OK] * 20
        assert np.array_equal(d_in.cpu().numpy().view(np.uint64), want[pick])
    pr.close()


def test_host_form_leaves_stride_padding_alone(gpu, squares5):
    """p25_p3_prove_batch with input_stride_words = num_inputs + 3 into a pre-filled array: the three words behind every
    proof keep what they held, the proofs are the packed call's."""
    air, traces, want = squares5
    pr = gpu.P3Prover(air, 5, 1, 6, 10)
    ni, stride, fill = pr.num_inputs, pr.num_inputs + 3, 0xA5A5A5A5A5A5A5A5
    out = np.full((5, stride), fill, dtype=np.uint64)
    st = np.full(5, 77, dtype=np.int32)
    tr = np.ascontiguousarray(traces, dtype=np.uint64)
    ps = np.array(POW_STARTS, dtype=np.uint64)
    rc = gpu.lib().p25_p3_prove_batch(pr._h, tr.ctypes.data, 5, ps.ctypes.data, out.ctypes.data, stride, st.ctypes.data)
    assert rc == OK and st.tolist() == [OK] * 5
    assert np.array_equal(out[:, :ni], want)
    assert (out[:, ni:] == fill).all()
    got, st = pr.prove(traces, pow_starts=POW_STARTS, input_stride=stride)     # the binding's own form of it
    assert st.tolist() == [OK] * 5 and got.shape == (5, stride)
    assert np.array_equal(got[:, :ni], want) and not got[:, ni:].any()
    pr.close()


# ---------------------------------------------------------------------------------------------------------------------
# 8. chained into the outer prover on one stream, no host copy
# ---------------------------------------------------------------------------------------------------------------------
def test_chain_into_the_outer_prover(gpu, fib_circuit, fib_oracle, fib_inputs):
    import torch
    dev = torch.device("cuda", 0)
    pr = gpu.P3Prover(gpu.Air.fibonacci(), 6, 1, 100, 16)
    assert pr.num_inputs == int(fib_circuit.info.num_inputs)
    pw = int(fib_circuit.info.proof_words)
    trace = air_cases.fib_trace(6)
    d_trace = torch.from_numpy(trace.view(np.int64).copy()).to(dev)
    d_seeds = torch.tensor([1], dtype=torch.int64, device=dev)
    d_inputs, d_ist = Banded(pr.num_inputs), Banded32(1)
    d_proof, d_pst = Banded(pw), Banded32(1)
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    pr.prove_dev(d_trace.data_ptr(), trace.size, 1, 0, d_inputs.ptr, pr.num_inputs, d_ist.ptr, side.cuda_stream)
    fib_circuit.wait_stream(side.cuda_stream)
    fib_circuit.prove_dev(d_inputs.ptr, 1, d_seeds.data_ptr(), d_proof.ptr, pw, d_pst.ptr)
    fib_circuit.sync()
    side.synchronize()
    assert d_ist.get().tolist() == [OK] and d_pst.get().tolist() == [OK]
    assert np.array_equal(d_inputs.get(), fib_inputs)
    want, st = fib_circuit.prove(fib_inputs[None, :], seeds=[1])
    assert st.tolist() == [OK]
    proof = d_proof.get()
    assert np.array_equal(proof, want[0])
    assert fib_oracle.verify(proof)[0] == 0
    for b in (d_inputs, d_ist, d_proof, d_pst):
        b.assert_bands_intact()


# ---------------------------------------------------------------------------------------------------------------------
# 9. an independent acceptance check: the oracle's verifier circuit takes the GPU's proof, and not a changed one
# ---------------------------------------------------------------------------------------------------------------------
def test_oracle_verifier_circuit_accepts_the_gpu_proof(gpu, oracle):
    air = air_cases.cubic(gpu)
    pr = gpu.P3Prover(air, 5, 1, 3, 4)
    got, st = pr.prove(air_cases.cubic_trace(5))
    assert st.tolist() == [OK]
    c = gpu.Circuit.build_p3_verifier_air(pr.config, air)
    oc = oracle.load_circuit(c.to_blob())
    inp = got[0]
    assert oc.witness(inp, seed=0)[1] == 0
    bad = inp.copy()
    bad[10] = (int(bad[10]) + 1) % P
    assert oc.witness(bad, seed=0)[1] == 4
