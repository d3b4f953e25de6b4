"""The two small circuits the stage tests run on, as plain functions (the fixtures `small` of test_gpu_stages.py and
`rec_small` of test_gpu_recursion.py re-created for the modules that share them), and the row -> gate kind table."""
import numpy as np

P = 0xFFFFFFFF00000001


def build_small(p25, oracle):
    """plonky3-verifier circuit of a 2^3-row Fibonacci STARK: 2^10 rows, every gate kind of the fib-64 circuit (1-10).
    Host code only -- no device needed.  Returns (circuit, oracle circuit, satisfied witness)."""
    inp, cfg = p25.p3_prove_fibonacci(3, 3, 4)
    c = p25.Circuit.build_p3_verifier(cfg)
    oc = oracle.load_circuit(c.to_blob())
    wires, st, msg = oc.witness(inp, seed=3)
    assert st == 0, msg
    return c, oc, wires


def build_rec_small(gpu, oracle):
    """Depth-2 recursion over the and(x, y) gadget circuit: the verifier (2^12 rows) of a recursive verifier (2^11 rows);
    it holds every gate kind recursion adds (11-17).  Needs the device: the inner proofs are proved on it."""
    inner = gpu.Circuit.build_gadget(0, 0)
    x, y = 0x0123456789ABCDEF % P, 0x0FEDCBA987654321 % P
    inp = np.array([x, y, (x & y) % P], dtype=np.uint64)
    inner_proofs, st = inner.prove(inp[None, :], seeds=[5])
    assert st.tolist() == [0]
    outer1 = inner.build_recursive_verifier(1)
    p1, st = outer1.prove(inner_proofs[:1], seeds=[6])
    assert st.tolist() == [0]
    outer = outer1.build_recursive_verifier(1)
    oo = oracle.load_circuit(outer.to_blob())
    wires, st, msg = oo.witness(p1[0], seed=9)
    assert st == 0, msg
    return outer, oo, wires


def row_kinds(blob):
    """Gate kind of every row, from the circuit blob (magic, 32 header words, the gate table
    of header[14] entries x 4 words, header[10] FRI arity words, then u32[n])."""
    hdr = np.frombuffer(blob, dtype=np.uint64, count=32, offset=8)
    off = 8 + 32 * 8 + int(hdr[14]) * 32 + int(hdr[10]) * 8
    return np.frombuffer(blob, dtype=np.uint32, count=1 << int(hdr[0]), offset=off).copy()


def first_row_of_each_kind(blob):
    """{gate kind: first row holding it}, the no-op kind 0 left out."""
    kinds = row_kinds(blob)
    return {int(k): int(np.nonzero(kinds == k)[0][0]) for k in np.unique(kinds) if k != 0}
