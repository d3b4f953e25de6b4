#!/usr/bin/env python3
"""Records tests/golden/high_rate/shrink_gadget8_rate8.npz: the ORACLE's proofs of the (8, 10, 16) shrink circuit over
gadget 8 (2^11 rows, an LDE of 2^19 points) for seeds 0, 1, 2, with the inner proof they verify.  The oracle takes 20-30 s
for each, which a GPU test may not; tests/test_gpu_high_rate.py compares the device's proofs with these words and
tests/test_high_rate_cpu.py proves one of them again with the live oracle.  CPU only."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from conftest import Oracle, load_p25   # noqa: E402
import gadget_cases                     # noqa: E402

INNER_SEED, SEEDS, CONFIG = 1, (0, 1, 2), (8, 10, 16)


def main():
    p25, oracle = load_p25(), Oracle()
    _name, kind, param, inputs = [c for c in gadget_cases.cases() if c[1] == 8][0]
    inner = p25.Circuit.build_gadget(kind, param)
    oc = oracle.load_circuit(inner.to_blob())
    pi, st, _tm, msg = oc.prove(np.array(inputs, dtype=np.uint64), seed=INNER_SEED)
    assert st == 0, msg
    so = oracle.load_circuit(inner.build_shrink(CONFIG, *oc.digest()).to_blob())
    proofs = []
    for seed in SEEDS:
        p, st, _tm, msg = so.prove(pi, seed=seed)
        assert st == 0 and so.verify(p)[0] == 0, msg
        proofs.append(p)
    out = os.path.join(ROOT, "tests", "golden", "high_rate", "shrink_gadget8_rate8.npz")
    os.makedirs(os.path.dirname(out), exist_ok=True)
    np.savez_compressed(out, inner_seed=np.uint64(INNER_SEED), inner_proof=pi, seeds=np.array(SEEDS, dtype=np.uint64),
                        proofs=np.stack(proofs))
    print(out, os.path.getsize(out), "bytes;", len(SEEDS), "proofs of", so.proof_words, "words")


if __name__ == "__main__":
    main()
