"""GPU: proofs go to the proving contexts by a running per-circuit counter (prover.hip, inflight.h), so the first context of a
witness pass rotates from pass to pass and from call to call.  Whatever context proves a proof, and whichever subset of
the contexts a short pass touches, every proof is byte for byte the oracle's and the one proved at depth 1."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_SEEDS = 7     # an oracle proof takes half a second: seven distinct proofs, 7 coprime to every depth and to the pass of 64
SIZES = [1, 5, 23, 24, 25, 63, 64, 65, 130]     # 65 and 130 cross a witness pass of 64; their last pass holds 1 and 2 proofs
DEPTHS = [3, 16, 24, 32]


def _gadget(oracle, name):
    from gadget_cases import cases
    _n, kind, param, vals = [c for c in cases(oracle) if c[0] == name][0]
    return kind, param, np.array(vals, dtype=np.uint64)


def _seeds(n, shift):
    """Seeds of a batch of n: proof i takes seed (i + shift) mod N_SEEDS.  Calls that follow each other on one circuit take
    different shifts, so a witness slot read before its pass has finished holds another proof's values, not the right ones."""
    return [(i + shift) % N_SEEDS for i in range(n)]


def _oracle_proofs(oracle, circuit, inp, n=N_SEEDS):
    oc = oracle.load_circuit(circuit.to_blob())
    out = []
    for seed in range(n):
        po, sto, _t, msg = oc.prove(inp, seed=seed)
        assert sto == 0, msg
        out.append(po)
    return np.stack(out)


@pytest.fixture(scope="module")
def ref(gpu, oracle):
    """The "compress" gadget circuit: the oracle's proofs of seeds 0..6 and the same proofs proved one at a time."""
    kind, param, inp = _gadget(oracle, "compress")
    c = gpu.Circuit.build_gadget(kind, param)
    c.set_streams(1)
    lone, st = c.prove(np.stack([inp] * N_SEEDS), seeds=list(range(N_SEEDS)))
    assert st.tolist() == [0] * N_SEEDS
    want = _oracle_proofs(oracle, c, inp)
    c.close()
    want.setflags(write=False)
    lone.setflags(write=False)
    circuits = {}      # depth -> the circuit that serves every batch size at that depth
    yield dict(kind=kind, param=param, inp=inp, oracle=want, lone=lone, circuits=circuits)
    for c in circuits.values():
        c.close()


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("depth", DEPTHS)
def test_batches_at_every_depth_equal_the_oracle_and_depth_1(gpu, ref, depth, n):
    """One circuit per depth serves all its batch sizes in turn, so the running counter stands somewhere else at the start of
    each: 1, 6, 29, 53, ... proofs in."""
    c = ref["circuits"].get(depth)
    if c is None:
        c = ref["circuits"][depth] = gpu.Circuit.build_gadget(ref["kind"], ref["param"])
        c.set_streams(depth)
    seeds = _seeds(n, SIZES.index(n))
    proofs, st = c.prove(np.stack([ref["inp"]] * n), seeds=seeds)
    assert st.tolist() == [0] * n
    bad = [i for i in range(n) if (proofs[i] != ref["oracle"][seeds[i]]).any()]
    assert not bad, f"proofs {bad[:8]} differ from the oracle's"
    assert (proofs == ref["lone"][seeds]).all()


def test_two_calls_without_a_synchronisation_between_them(gpu, ref):
    """Two device-resident calls of 5 proofs at depth 24, only enqueued: the counter goes on from the first call into the
    second, the second call's witness pass runs under the first call's proofs."""
    import torch
    dev = torch.device("cuda", 0)
    c = gpu.Circuit.build_gadget(ref["kind"], ref["param"])
    c.set_streams(24)
    pw, n = int(c.info.proof_words), 5
    d_in = torch.from_numpy(np.stack([ref["inp"]] * n).view(np.int64)).to(dev)
    seeds = [_seeds(n, 0), _seeds(n, 3)]
    d_seeds = [torch.tensor(sd, dtype=torch.int64, device=dev) for sd in seeds]
    d_p = torch.zeros((2, n, pw), dtype=torch.int64, device=dev)
    d_s = torch.ones((2, n), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    for k in range(2):
        c.prove_dev(d_in.data_ptr(), n, d_seeds[k].data_ptr(), d_p[k].data_ptr(), pw, d_s[k].data_ptr())
    c.sync(); torch.cuda.synchronize()
    assert d_s.cpu().tolist() == [[0] * n] * 2
    got = d_p.cpu().numpy().view(np.uint64).reshape(2 * n, pw)
    assert (got == ref["oracle"][seeds[0] + seeds[1]]).all()
    c.close()


def test_two_circuits_interleave_batches_on_the_shared_pool(gpu, oracle, ref):
    """Two live circuits at depth 24 on the one stream pool, a.prove_dev / b.prove_dev alternating with no synchronisation,
    in sizes that leave each circuit's counter at a different place every time."""
    import torch
    dev = torch.device("cuda", 0)
    sizes = [5, 25, 65]
    total = sum(sizes)
    seeds = _seeds(sizes[0], 1) + _seeds(sizes[1], 2) + _seeds(sizes[2], 4)
    kb, pb, inp_b = _gadget(oracle, "and")
    circ = {"compress": (gpu.Circuit.build_gadget(ref["kind"], ref["param"]), ref["inp"], ref["oracle"]),
            "and": (gpu.Circuit.build_gadget(kb, pb), inp_b, None)}
    bufs = {}
    for name, (c, inp, _w) in circ.items():
        c.set_streams(24)
        pw = int(c.info.proof_words)
        bufs[name] = dict(pw=pw, d_in=torch.from_numpy(np.stack([inp] * total).view(np.int64)).to(dev),
                          d_seeds=torch.tensor(seeds, dtype=torch.int64, device=dev),
                          d_p=torch.zeros((total, pw), dtype=torch.int64, device=dev),
                          d_s=torch.ones((total,), dtype=torch.int32, device=dev))
    torch.cuda.synchronize()
    base = 0
    for n in sizes:
        for name, (c, _i, _w) in circ.items():
            b = bufs[name]
            c.prove_dev(b["d_in"].data_ptr(), n, b["d_seeds"][base:].data_ptr(), b["d_p"][base:].data_ptr(), b["pw"],
                        b["d_s"][base:].data_ptr())
        base += n
    for c, _i, _w in circ.values():
        c.sync()
    torch.cuda.synchronize()
    for name, (c, inp, want) in circ.items():
        b = bufs[name]
        assert int((b["d_s"] != 0).sum().item()) == 0, name
        if want is None:
            want = _oracle_proofs(oracle, c, inp)
        got = b["d_p"].cpu().numpy().view(np.uint64)
        bad = [i for i in range(total) if (got[i] != want[seeds[i]]).any()]
        assert not bad, (name, bad[:8])
        c.close()


def test_one_live_circuit_grows_from_1_to_3_to_24_contexts(gpu, ref):
    """set_streams(1) and 1 proof, set_streams(3) and 5, set_streams(24) and 25, on one circuit that is never closed in
    between: its contexts are built 0 -> 1 -> 3 -> 24 beside the ones already proving, and its share of the stream pool
    is reserved once and widened twice.  Every proof is the oracle's for its seed."""
    c = gpu.Circuit.build_gadget(ref["kind"], ref["param"])
    try:
        for step, (depth, n) in enumerate([(1, 1), (3, 5), (24, 25)]):
            c.set_streams(depth)
            seeds = _seeds(n, step)
            proofs, st = c.prove(np.stack([ref["inp"]] * n), seeds=seeds)
            assert st.tolist() == [0] * n, (depth, n)
            bad = [i for i in range(n) if (proofs[i] != ref["oracle"][seeds[i]]).any()]
            assert not bad, f"depth {depth}: proofs {bad[:8]} differ from the oracle's"
    finally:
        c.close()


def test_phase_timings_of_one_proof(gpu, ref):
    """prove(timings=True): the proof is the oracle's, and the nine phase times (HIP events that live for the call or
    belong to the context) are finite, non-negative, and none exceeds the total."""
    c = gpu.Circuit.build_gadget(ref["kind"], ref["param"])
    try:
        proofs, st, tm = c.prove(ref["inp"][None, :], seeds=[3], timings=True)
    finally:
        c.close()
    assert st.tolist() == [0]
    assert (proofs[0] == ref["oracle"][3]).all()
    t = tm.as_dict()
    print("phase ms:", {k: round(v, 4) for k, v in t.items()})
    assert len(t) == 9 and "total_ms" in t
    assert all(np.isfinite(v) and v >= 0 for v in t.values()), t
    assert all(t["total_ms"] >= v for v in t.values()), t
