"""CPU: circuits under high-rate FRI configs (rate_bits 4..8) on the host side -- the blob importer, the config entry
points (p25_circuit_config_of, p25_circuit_build_gadget_cfg, p25_circuit_build_shrink) and the shrink chain, with the
oracle as the prover and verifier: it proves and verifies any rate (its quotient is evaluated on the whole LDE).

The recorded rate-8 proofs of tests/golden/high_rate/ (what tests/test_gpu_high_rate.py compares the device with, because
the oracle takes 20-30 s for each) are checked here against the live oracle."""
import ctypes as C
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import gadget_cases
import high_rate as hr
from conftest import P, ROOT

INVALID_ARG, WITNESS_CONFLICT = 1, 4
GOLD = os.path.join(ROOT, "tests", "golden", "high_rate")


def test_blob_with_rate_bits_5_imports_and_config_reads_it_back(p25, oracle):
    c = p25.Circuit.build_gadget(11, 3)
    assert c.config.as_tuple() == hr.STANDARD and c.config.conjectured_security_bits == 100
    blob = c.to_blob()
    assert hr.header(blob)[6] == 3
    c5 = p25.Circuit.from_blob(hr.rewrite_config(blob, 5))
    assert c5.config.as_tuple() == (5, 28, 16)
    assert hr.header(c5.to_blob())[6] == 5 and c5.to_blob() == hr.rewrite_config(blob, 5)
    # every rate up to 8 with its query count, and the proof gets shorter as the queries fall
    words = [int(c.info.proof_words)]
    for rate in (4, 5, 6, 7, 8):
        k = p25.Circuit.from_blob(hr.rewrite_config(blob, rate, hr.QUERIES[rate]))
        assert k.config.as_tuple() == (rate, hr.QUERIES[rate], 16)
        assert int(k.info.proof_words) == oracle.load_circuit(k.to_blob()).proof_words
        words.append(int(k.info.proof_words))
    assert words == sorted(words, reverse=True) and len(set(words)) == len(words)


def test_blob_rates_refused_by_name(p25):
    blob = p25.Circuit.build_gadget(11, 3).to_blob()
    for bad, name in ((hr.rewrite_config(blob, 9), "rate_bits must be in 0..8"),
                      (hr.rewrite_config(blob, 8, h0=17, fix_arity=False), "degree_bits + rate_bits"),     # 17 + 8 = 25
                      (hr.rewrite_config(blob, 3, h0=22, fix_arity=False), "degree_bits + rate_bits"),     # 22 + 3 = 25
                      (hr.rewrite_config(blob, 2), "max_quotient_degree_factor"),                            # factor 8, rate 2
                      (hr.rewrite_config(blob, 5, h5=32, h13=2), "max_quotient_degree_factor")):             # factor 2^rate above 3
        with pytest.raises(p25.P25Error) as e:
            p25.Circuit.from_blob(bad)
        assert e.value.status == INVALID_ARG and name in str(e.value), str(e.value)


@pytest.mark.parametrize("kind,param", [(8, 0), (11, 3), (14, 0)])
def test_gadget_cfg_standard_is_the_plain_builder_byte_for_byte(p25, kind, param):
    lib = p25.lib()
    plain = p25.Circuit.build_gadget(kind, param).to_blob()
    h = C.c_void_p()
    assert lib.p25_circuit_build_gadget_cfg(kind, param, None, C.byref(h)) == 0
    assert p25.Circuit(h.value).to_blob() == plain
    assert p25.Circuit.build_gadget(kind, param, hr.STANDARD).to_blob() == plain
    assert p25.Circuit.build_gadget(kind, param, p25.CircuitConfig()).to_blob() == plain
    # another config changes the three header words (and nothing else at a size without FRI layers)
    other = p25.Circuit.build_gadget(kind, param, (7, 12, 10)).to_blob()
    assert other != plain and other == hr.rewrite_config(plain, 7, 12, 10)


def test_every_out_of_range_config_field_is_invalid_arg(p25):
    lib = p25.lib()
    inner = p25.Circuit.build_gadget(8, 0)
    dg, cap = np.zeros(4, dtype=np.uint64), np.zeros(64, dtype=np.uint64)
    bad = {"rate_bits": [(2, 28, 16, 0), (9, 28, 16, 0), (-1, 28, 16, 0)],
           "num_query_rounds": [(3, 0, 16, 0), (3, 65, 16, 0), (8, -3, 16, 0)],
           "proof_of_work_bits": [(3, 28, -1, 0), (3, 28, 33, 0)],
           "reserved": [(3, 28, 16, 1), (8, 10, 16, -1)]}
    for field, configs in bad.items():
        for cfg in configs:
            cc = p25.CircuitConfig(*cfg)
            for call in (lambda h: lib.p25_circuit_build_gadget_cfg(8, 0, C.byref(cc), C.byref(h)),
                         lambda h: lib.p25_circuit_build_shrink(inner._h, dg.ctypes.data_as(C.c_void_p),
                                                                cap.ctypes.data_as(C.c_void_p), C.byref(cc), C.byref(h))):
                h = C.c_void_p()
                assert call(h) == INVALID_ARG and not h.value, (field, cfg)
                assert field in lib.p25_last_error().decode(), (field, cfg, lib.p25_last_error())
    # the extremes of every range are accepted
    for cfg in ((3, 1, 0), (8, 64, 32)):
        assert p25.Circuit.build_gadget(8, 0, cfg).config.as_tuple() == cfg
    assert lib.p25_circuit_config_of(None, C.byref(p25.CircuitConfig())) == INVALID_ARG
    assert lib.p25_circuit_config_of(inner._h, None) == INVALID_ARG


def test_cfg_blobs_carry_the_arity_list_of_the_upstream_rule(p25, oracle):
    """fri_reduction_arity_bits follows the config: ConstantArityBits(4, 5) folds while the polynomial is longer than 2^5
    and the next layer still has a leaf per cap entry.  The gadget circuits (at most 2^5 rows) never fold; the shrink
    circuits (2^11 rows) fold twice."""
    seen = set()
    cases = [(kind, param) for _n, kind, param, _i in gadget_cases.cases(oracle)] + [(7, 16), (10, 200), (11, 64)]
    for kind, param in cases:
        for rate in (3, 4, 6, 8):
            blob = p25.Circuit.build_gadget(kind, param, (rate, hr.QUERIES[rate], 16)).to_blob()
            h = hr.header(blob)
            assert hr.arity_list(blob) == hr.arity_rule(h[0], rate), (kind, param, rate)
            seen.add((h[0], len(hr.arity_list(blob))))
    inner = p25.Circuit.build_gadget(8, 0)
    vd = oracle.load_circuit(inner.to_blob()).digest()
    for rate in (3, 4, 5, 6, 7, 8):
        blob = inner.build_shrink((rate, hr.QUERIES[rate], 16), *vd).to_blob()
        h = hr.header(blob)
        assert h[0] == 11 and hr.arity_list(blob) == hr.arity_rule(11, rate) == [4, 4], rate
        seen.add((h[0], 2))
    assert {n for _db, n in seen} == {0, 2}
    # the rule itself where the rate decides (below what the builders take): 2^6 rows fold at rate 2, not at rate 1
    assert hr.arity_rule(6, 2) == [4] and hr.arity_rule(6, 1) == [] and hr.arity_rule(12, 8) == [4, 4]


@pytest.fixture(scope="module")
def chain(p25, oracle):
    """gadget 11 (param 3: five public inputs) proved by the oracle, then the two shrink steps (7, 12, 16) and (8, 10, 16),
    each built from the oracle's verifier data of the step below and proved by the oracle from the proof below."""
    inner = p25.Circuit.build_gadget(11, 3)
    oc = oracle.load_circuit(inner.to_blob())
    proof, st, _tm, msg = oc.prove(np.array(hr.public_inputs_gadget_inputs(3), dtype=np.uint64), seed=1)
    assert st == 0, msg
    steps = [dict(circuit=inner, oc=oc, proof=proof, vd=oc.digest())]
    for cfg in hr.SHRINK_CHAIN:
        below = steps[-1]
        c = below["circuit"].build_shrink(cfg, *below["vd"])
        so = oracle.load_circuit(c.to_blob())
        p, st, _tm, msg = so.prove(below["proof"], seed=2)
        assert st == 0, msg
        steps.append(dict(circuit=c, oc=so, proof=p, vd=so.digest(), cfg=cfg))
    return steps


def test_shrink_chain_is_proved_and_verified_by_the_oracle(p25, chain):
    inner = chain[0]
    pis = inner["circuit"].public_inputs(inner["proof"])
    xs = hr.public_inputs_gadget_inputs(3)
    assert pis.tolist() == xs + [xs[0] * xs[1] % P, xs[0] * xs[1] * xs[2] % P]
    # a standard-config shrink of the same proof: what every step is compared with
    std = inner["circuit"].build_shrink(None, *inner["vd"])
    assert std.config.as_tuple() == hr.STANDARD and int(std.info.num_public_inputs) == 5
    assert std.to_blob() == inner["circuit"].build_shrink(hr.STANDARD, *inner["vd"]).to_blob()
    words = [int(std.info.proof_words)]
    for below, step in zip(chain, chain[1:]):
        c, so = step["circuit"], step["oc"]
        assert c.config.as_tuple() == step["cfg"] and int(c.info.num_public_inputs) == 5
        assert int(c.info.num_inputs) == int(below["circuit"].info.proof_words) == below["proof"].size
        assert hr.arity_list(c.to_blob()) == hr.arity_rule(int(c.info.degree_bits), step["cfg"][0])
        assert so.verify(step["proof"], *step["vd"])[0] == 0
        assert c.public_inputs(step["proof"]).tolist() == pis.tolist()            # the same words in the same order
        for w in (0, 300, below["proof"].size - 6, below["proof"].size - 1):       # a cap word, an opening, PoW witness, a public input
            bad = below["proof"].copy()
            bad[w] ^= np.uint64(1)
            assert so.prove(bad, seed=2)[1] == WITNESS_CONFLICT, w
        words.append(int(c.info.proof_words))
    assert words[0] > words[1] > words[2], words                                  # strictly shorter at each step
    # it verifies exactly what the recursive verifier of one proof verifies: same rows but for the public-input gate
    rv = inner["circuit"].build_recursive_verifier(1, *inner["vd"])
    assert int(rv.info.num_public_inputs) == 0 and int(rv.info.num_inputs) == int(std.info.num_inputs)
    assert abs(int(std.info.num_rows_used) - int(rv.info.num_rows_used)) <= 2


def test_shrink_of_a_circuit_without_public_inputs_registers_none(p25, oracle):
    inner = p25.Circuit.build_gadget(8, 0)
    vd = oracle.load_circuit(inner.to_blob()).digest()
    s = inner.build_shrink((8, 10, 16), *vd)
    rv = inner.build_recursive_verifier(1, *vd)
    assert int(s.info.num_public_inputs) == 0 and int(s.info.num_rows_used) == int(rv.info.num_rows_used)
    assert hr.rewrite_config(rv.to_blob(), 8, 10, 16) == s.to_blob()   # the recursive verifier of one proof, under the config


def test_proof_formats_round_trip_a_rate_8_proof(p25, chain):
    c, proof = chain[2]["circuit"], chain[2]["proof"]
    assert c.config.as_tuple() == (8, 10, 16)
    raw = c.proof_to_bytes(proof)
    assert (c.proof_from_bytes(raw) == proof).all()
    js = json.loads(c.proof_to_json(proof))
    assert len(js["proof"]["opening_proof"]["query_round_proofs"]) == 10
    assert (hr.flatten_proof_json(js) == proof).all()
    depth = int(c.info.degree_bits) + 8 - hr.CAP_HEIGHT
    assert len(js["proof"]["opening_proof"]["query_round_proofs"][0]["initial_trees_proof"]["evals_proofs"][0][1]["siblings"]) == depth


def test_recorded_rate_8_shrink_proofs_are_the_oracles(p25, oracle):
    """tests/golden/high_rate/shrink_gadget8_rate8.npz: the oracle's proofs of the (8, 10, 16) shrink circuit over gadget 8
    for seeds 0, 1, 2 (tools/record_high_rate_golden.py).  Seed 1 is proved again here; all three verify."""
    gold = np.load(os.path.join(GOLD, "shrink_gadget8_rate8.npz"))
    name, kind, param, inputs = [c for c in gadget_cases.cases() if c[1] == 8][0]
    inner = p25.Circuit.build_gadget(kind, param)
    oc = oracle.load_circuit(inner.to_blob())
    pi, st, _tm, msg = oc.prove(np.array(inputs, dtype=np.uint64), seed=int(gold["inner_seed"]))
    assert st == 0 and (pi == gold["inner_proof"]).all(), msg
    s = inner.build_shrink((8, 10, 16), *oc.digest())
    so = oracle.load_circuit(s.to_blob())
    assert gold["proofs"].shape == (3, so.proof_words) and gold["seeds"].tolist() == [0, 1, 2]
    for p in gold["proofs"]:
        assert so.verify(p)[0] == 0
    p1, st, _tm, msg = so.prove(pi, seed=1)
    assert st == 0 and (p1 == gold["proofs"][1]).all(), msg


def test_ntt_index_maps_at_the_high_rate_extremes(tmp_path):
    """tests/native/ntt_index_high_rate.cpp: the cursors of both LDE passes in 32-bit arithmetic against 64-bit closed
    forms for B up to 2^24 words, the block decode with 16..256 cosets, the coset blocks."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "ntt_index_high_rate")
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"),
                        os.path.join(ROOT, "tests", "native", "ntt_index_high_rate.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "NTT INDEX HIGH RATE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]


def test_working_set_of_a_high_rate_circuit_sizes_the_quotient_by_its_own_coset(tmp_path):
    """tests/native/working_set_high_rate.cpp: up to rate 3 every buffer is what it was; above it the three quotient
    buffers hold 8n words per challenge while everything committed grows with the LDE."""
    gxx = shutil.which("g++")
    if not gxx:
        pytest.skip("g++ not available")
    exe = str(tmp_path / "working_set_high_rate")
    r = subprocess.run([gxx, "-std=c++17", "-O2", "-Wall", "-I" + os.path.join(ROOT, "plonky2.5_amd", "csrc"),
                        "-I" + os.path.join(ROOT, "tests", "native", "fake_hip"),
                        os.path.join(ROOT, "tests", "native", "working_set_high_rate.cpp"), "-o", exe], capture_output=True, text=True,
                       timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "WORKING SET HIGH RATE OK" in r.stdout, r.stdout[-2000:] + r.stderr[-500:]
