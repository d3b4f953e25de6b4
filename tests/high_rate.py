"""What the high-rate tests share (tests/test_high_rate_cpu.py on the host, tests/test_gpu_high_rate.py on the GPU): the
configs, upstream's FRI arity rule restated, a blob rewritten to another config, serde JSON back to flat words."""
import struct

import numpy as np

P = 0xFFFFFFFF00000001
# rate_bits -> num_query_rounds at 16 proof-of-work bits: the smallest count with rate_bits * queries + 16 >= 100
QUERIES = {3: 28, 4: 21, 5: 17, 6: 14, 7: 12, 8: 10}
STANDARD = (3, 28, 16)
SHRINK_CHAIN = ((7, 12, 16), (8, 10, 16))
HEADER_WORDS, ARITY_BITS, FINAL_POLY_BITS, CAP_HEIGHT = 32, 4, 5, 4


def arity_rule(degree_bits, rate_bits, arity_bits=ARITY_BITS, final_poly_bits=FINAL_POLY_BITS, cap_height=CAP_HEIGHT):
    """upstream FriReductionStrategy::ConstantArityBits(arity_bits, final_poly_bits).reduction_arity_bits(degree_bits,
    rate_bits, cap_height, ..): fold while the polynomial is longer than 2^final_poly_bits and the next layer's LDE still
    has a leaf per cap entry."""
    out, db = [], degree_bits
    while db > final_poly_bits and db + rate_bits - arity_bits >= cap_height:
        out.append(arity_bits)
        db -= arity_bits
    return out


def header(blob):
    return list(struct.unpack_from(f"<{HEADER_WORDS}Q", blob, 8))


def arity_list(blob):
    h = header(blob)
    off = 8 + 8 * HEADER_WORDS + 32 * h[14]
    return list(struct.unpack_from(f"<{h[10]}Q", blob, off))


def rewrite_config(blob, rate_bits, num_query_rounds=None, proof_of_work_bits=None, fix_arity=True, **words):
    """The blob with header word 6 (rate_bits), 9 (num_query_rounds) and 8 (proof_of_work_bits) rewritten, any other header
    word by its index (h5=4), and -- a blob being what a builder under that config would have written -- the arity list
    that the rule gives at the new rate."""
    h = header(blob)
    off = 8 + 8 * HEADER_WORDS + 32 * h[14]
    tail = blob[off + 8 * h[10]:]
    arity = arity_list(blob)
    h[6] = rate_bits
    if num_query_rounds is not None:
        h[9] = num_query_rounds
    if proof_of_work_bits is not None:
        h[8] = proof_of_work_bits
    for k, v in words.items():
        h[int(k[1:])] = v
    if fix_arity:
        arity = arity_rule(h[0], rate_bits, h[20], h[21], h[7])
        h[10] = len(arity)
    return blob[:8] + struct.pack(f"<{HEADER_WORDS}Q", *h) + blob[8 + 8 * HEADER_WORDS:off] + struct.pack(f"<{len(arity)}Q", *arity) + tail


def flatten_proof_json(js):
    """serde JSON of ProofWithPublicInputs -> the flat word layout of include/p25.h, public inputs last."""
    out, pr = [], js["proof"]

    def cap(c):
        for hh in c:
            out.extend(int(x) for x in hh["elements"])

    def exts(v):
        for e in v:
            out.extend(int(x) for x in e)

    cap(pr["wires_cap"]); cap(pr["plonk_zs_partial_products_cap"]); cap(pr["quotient_polys_cap"])
    for k in ("constants", "plonk_sigmas", "wires", "plonk_zs", "plonk_zs_next", "partial_products", "quotient_polys"):
        exts(pr["openings"][k])
    fp = pr["opening_proof"]
    for c in fp["commit_phase_merkle_caps"]:
        cap(c)
    for q in fp["query_round_proofs"]:
        for leaf, path in q["initial_trees_proof"]["evals_proofs"]:
            out.extend(int(x) for x in leaf)
            cap(path["siblings"])
        for step in q["steps"]:
            exts(step["evals"])
            cap(step["merkle_proof"]["siblings"])
    exts(fp["final_poly"]["coeffs"])
    out.append(int(fp["pow_witness"]))
    out.extend(int(x) for x in js["public_inputs"])
    return np.array(out, dtype=np.uint64)


def public_inputs_gadget_inputs(k=3):
    """Inputs of gadget 11 with param k: x_0 .. x_{k-1}; it exposes them and their k - 1 running products."""
    return [(0x9E3779B97F4A7C15 * (i + 1)) % P for i in range(k)]
