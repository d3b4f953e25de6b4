#!/usr/bin/env python3
"""What the last proof of an aggregation costs to shrink, on the GPU: an aggregated fib-64 root (`--leaves` verifier
proofs folded `--arity` at a time) is put through
  standard   one shrink step under the standard recursion config (3, 28, 16), and
  chain      the two steps (7, 12, 16) then (8, 10, 16) of upstream's size-optimised recursion,
and for every step the circuit's rows, the proof's bytes (upstream's ProofWithPublicInputs::to_bytes) and the device time
of one proof from HIP events (p25_prove_batch's timings: median of `--repeats` after a warm-up proof) are recorded.
Every proof is checked: the library's verifier accepts it and it carries the root's public inputs.
Record only, no threshold.  Writes one JSON document (default profiles/high_rate_shrink.json).
usage: shrink_bench.py [--leaves 8] [--arity 8] [--repeats 5] [--out PATH]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def step(p25, name, below_circuit, below_proof, cfg, repeats, pis):
    t = time.perf_counter()
    c = below_circuit.build_shrink(cfg)
    c.digest()
    build_s = time.perf_counter() - t
    inp = np.ascontiguousarray(below_proof, dtype=np.uint64)[None, :]
    out, st = c.prove(inp, seeds=[0])                     # warm-up: the circuit's context, tables and code objects
    assert st.tolist() == [0], st
    ms, phases = [], None
    for r in range(repeats):
        out, st, tm = c.prove(inp, seeds=[0], timings=True)
        assert st.tolist() == [0], st
        ms.append(tm.total_ms)
        phases = tm.as_dict()
    proof = out[0].copy()
    assert c.verify(proof[None, :]).tolist() == [0], "the library's verifier rejects the proof"
    assert c.public_inputs(proof).tolist() == pis, "public inputs changed"
    cc = c.config
    rec = {"step": name, "config": list(cc.as_tuple()), "conjectured_security_bits": cc.conjectured_security_bits,
           "rows_used": int(c.info.num_rows_used), "degree_bits": int(c.info.degree_bits),
           "lde_bits": int(c.info.degree_bits) + int(cc.rate_bits), "proof_words": int(c.info.proof_words),
           "proof_bytes": len(c.proof_to_bytes(proof)), "prove_ms_median": round(statistics.median(ms), 3),
           "prove_ms_min": round(min(ms), 3), "prove_ms_max": round(max(ms), 3), "repeats": repeats,
           "phases_ms_last": {k: round(v, 3) for k, v in phases.items()}, "circuit_build_s": round(build_s, 2)}
    return c, proof, rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--leaves", type=int, default=8)
    ap.add_argument("--arity", type=int, default=8)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "high_rate_shrink.json"))
    a = ap.parse_args()
    import __graft_entry__ as ge
    p25 = ge.load_package()
    from plonky25_amd import aggregate as ag
    p25.device_init(0)
    with open(os.path.join(ROOT, "tests", "golden", "proof_fibonacci.json")) as f:
        base, cfg = p25.p3_proof_from_json(f.read())
    leaf = p25.Circuit.build_p3_verifier(cfg)
    leaf.digest()
    leaves, st = leaf.prove(np.stack([base] * a.leaves), seeds=list(range(a.leaves)))
    assert (st == 0).all()
    fold = ag.fold(leaf, [leaves[i] for i in range(a.leaves)], arity=a.arity)
    top, root = fold["top"], fold["root"]
    pis = top.public_inputs(root).tolist()
    doc = {"what": "shrinking an aggregated fib-64 root: one standard-config step against the (7,12,16) -> (8,10,16) chain",
           "leaves": a.leaves, "arity": a.arity,
           "root": {"config": list(top.config.as_tuple()), "rows_used": int(top.info.num_rows_used),
                    "degree_bits": int(top.info.degree_bits), "proof_words": int(top.info.proof_words),
                    "proof_bytes": len(top.proof_to_bytes(root)), "public_inputs": pis},
           "standard": [], "chain": []}
    c, _p, rec = step(p25, "standard", top, root, None, a.repeats, pis)
    doc["standard"].append(rec)
    c.close()
    circ, proof, owned = top, root, []
    for i, cfg_i in enumerate(ag.SHRINK_CONFIGS):
        circ, proof, rec = step(p25, f"chain {i + 1}", circ, proof, cfg_i, a.repeats, pis)
        owned.append(circ)
        doc["chain"].append(rec)
    doc["chain_total_ms_median"] = round(sum(r["prove_ms_median"] for r in doc["chain"]), 3)
    doc["final_proof_bytes"] = {"root": doc["root"]["proof_bytes"], "standard": doc["standard"][0]["proof_bytes"],
                                "chain": doc["chain"][-1]["proof_bytes"]}
    for c in owned + fold["owned"] + [leaf]:
        c.close()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(doc, f, indent=1)
        f.write("\n")
    print(json.dumps(doc))


if __name__ == "__main__":
    main()
