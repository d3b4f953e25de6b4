"""What tests/test_quotient_model_cpu.py (the oracle, on the host) and tests/test_gpu_quotient_model.py (the device) share:
the circuits of tests/witgen_cases.py under their standard and other configurations, their twins with one PoseidonMds row,
the wire fills and challenges every circuit is run on, and the results of the Python model (tests/quotient_model.py), computed
once a process.

A data set is (label, wires, betas, gammas, alphas).  The labels are fixed here, so both files run the same sets; the CPU file
asserts that the model's partial products meet no zero denominator on any of them.
"""
import numpy as np

import blob_writer as bw
import edge_values as ev
import gate_models as gm
import quotient_model as qm
import witgen_cases as wc
from edge_values import EPS, P

BUILDER = dict(zip(wc.NAMES, wc.BUILDERS))
BOUNDARY = [0, 1, P - 1, EPS]                          # 0, 1, p - 1, 2^32 - 1

# (num_wires, num_routed, rate_bits) beside the standard (135, 80, 3): NP = 7, 10 (a last chunk of 4 wires) and 15; a row of
# exactly the 80 wires the merged pass reads, and one with 65 columns behind the gates' wires; a rate above the quotient's
CONFIGS = [(135, 64, 3), (135, 84, 3), (135, 128, 3), (80, 80, 3), (200, 80, 3), (135, 80, 4)]
CONFIG_CASES = ["arithmetic", "low_high", "mul_extension", "quotient_extension"]
# blobs the library must refuse: (label, config, case, what the message says)
REFUSED = [("more routed wires than the kernels hold", (200, 136, 3), "arithmetic", "bad wire counts"),
           ("three constant polynomials", (135, 80, 3, 3), "arithmetic", "num_constants must be 2"),
           ("ArithmeticGate on 64 wires", (64, 64, 3), "arithmetic", "more wires than the circuit has"),
           ("MulExtensionGate on 72 wires", (72, 64, 3), "mul_extension", "more wires than the circuit has")]
SUB_CASES = ["arithmetic", "reducing_extension"]      # run at rate_bits 4 (the _sub kernels)


class Circuit:
    """A case of witgen_cases under a configuration: its MiniCircuit, the build() dictionary, the blob."""

    def __init__(self, name, config=(bw.NUM_WIRES, bw.NUM_ROUTED, 3), twin=False):
        self.name, self.config, self.twin = name, config, twin
        standard = config == (bw.NUM_WIRES, bw.NUM_ROUTED, 3)
        if name in TINY:
            assert standard and not twin
            self.case = TINY[name]()
        elif standard and not twin:
            self.case = wc.all_cases()[name]
        else:
            kw = {} if standard else dict(num_wires=config[0], num_routed=config[1], rate_bits=config[2])
            self.case = BUILDER[name](**kw)
        self.extra_inputs = 0
        mc = self.case.circuit
        if twin:            # one PoseidonMds row on inputs of its own: the circuit is then proved by the recursion kernels
            assert max(self.case.gates) < bw.G_ARITH_EXT
            mc.poseidon_mds(wc.pairs([mc.input() for _ in range(24)]))
            self.extra_inputs = 24
        self.b = mc.build()
        self.blob = mc.to_blob() if (twin or not standard) else self.case.blob
        self.n = 1 << self.b["degree_bits"]
        assert self.n <= 64
        self.key = (name, config, twin)

    def inputs(self, row=0):
        """Inputs of a satisfied witness: operand row `row` of the case (a twin's PoseidonMds row reads edge words)."""
        inp = self.case.inputs(self.case.rows[row])
        return np.concatenate([inp, ev.edge(self.extra_inputs, 77)]) if self.extra_inputs else inp

    def rows_of(self, kind):
        return [r for r, row in enumerate(self.b["rows"]) if row[0] == kind]


def _tiny(build, n_ops, gate):
    """A circuit of one row of `gate` (and the PublicInput and Constant rows): 2^2 rows, for the tests that evaluate the
    model once per wire."""
    def make():
        c = bw.MiniCircuit()
        ins = [c.input() for _ in range(n_ops)]
        outs = build(c, ins)
        return wc.Case("tiny", c, n_ops, [], lambda ops: {}, [[3, 5, 7, 11, 13, 17][:n_ops]], set(), {gate}), outs
    return lambda: make()[0]


TINY = {"tiny_base_sum": _tiny(lambda c, i: c.range_check(i[0], 8), 1, bw.G_BASE_SUM),
        "tiny_arithmetic": _tiny(lambda c, i: c.arithmetic(3, 5, i[0], i[1], i[2]), 3, bw.G_ARITHMETIC),
        "tiny_arithmetic_extension": _tiny(lambda c, i: c.arithmetic_extension(3, 5, i[0:2], i[2:4], i[4:6]), 6, bw.G_ARITH_EXT)}
WITNESS_SEED = 5
_circuits = {}


def circuit(name, config=(bw.NUM_WIRES, bw.NUM_ROUTED, 3), twin=False):
    key = (name, config, twin)
    if key not in _circuits:
        _circuits[key] = Circuit(name, config, twin)
    return _circuits[key]


TWINS = [n for n in wc.NAMES if max(wc.all_cases()[n].gates) < bw.G_ARITH_EXT]
assert len(TWINS) == 9


# ---- data sets ---------------------------------------------------------------------------------------------------------------
def fills(c, witness=None):
    """(label, wires[num_wires][n]): the satisfied witness (if one is handed in) and the arbitrary fills."""
    W, n = c.config[0], c.n
    out = [] if witness is None else [("witness", np.ascontiguousarray(witness, dtype=np.uint64))]
    out.append(("edge", ev.edge(W * n, 21).reshape(W, n)))
    out.append(("mixed", ev.mixed(W * n, 22).reshape(W, n)))
    out.append(("const(p-1)", ev.const(W * n, P - 1).reshape(W, n)))
    return out


def boundary_challenges():
    """Four (label, betas, gammas, alphas): every one of 0, 1, p - 1, 2^32 - 1 as a beta, as a gamma and as an alpha.  A
    boundary beta sits in challenge 0 beside a uniform gamma and a boundary gamma in challenge 1 beside a uniform beta, so
    that w + beta sigma + gamma is zero nowhere on the fills below."""
    for k in range(4):
        u = ev.uniform(2, 60 + k)
        yield (f"boundary {k}", [BOUNDARY[k], int(u[0])], [int(u[1]), BOUNDARY[(k + 1) % 4]],
               [BOUNDARY[(k + 2) % 4], BOUNDARY[(k + 3) % 4]])


def data_sets(c, witness=None, boundary=True):
    """(label, wires, betas, gammas, alphas): every fill under uniform challenges, then the edge fill (seed 23) under the
    boundary challenges."""
    out = []
    for k, (label, wires) in enumerate(fills(c, witness)):
        ch = ev.uniform_challenges(40 + k)
        out.append((label, wires, [int(v) for v in ch[0]], [int(v) for v in ch[1]], [int(v) for v in ch[2]]))
    if boundary:
        W, n = c.config[0], c.n
        wires = ev.edge(W * n, 23).reshape(W, n)
        for label, betas, gammas, alphas in boundary_challenges():
            out.append((label, wires, betas, gammas, alphas))
    return out


# ---- the model's results, once a process --------------------------------------------------------------------------------------
_model = {}


def model(c, label, wires, betas, gammas, alphas):
    """(zs_pp, quotient) of the Python model as uint64 arrays; the quotient is evaluated on the model's own zs_pp."""
    key = (c.key, label, hash(np.ascontiguousarray(wires).tobytes()), tuple(betas), tuple(gammas), tuple(alphas))
    if key not in _model:
        zs = qm.partial_products(c.b, wires, betas, gammas)
        q = qm.quotient(c.b, wires, zs, betas, gammas, alphas)
        _model[key] = (np.array(zs, dtype=np.uint64), np.array(q, dtype=np.uint64))
    return _model[key]


def to_u64(m):
    return np.array(m, dtype=np.uint64)


BUMP_PART = 32                                         # wires bumped per case of the every-wire test


def bump_parts():
    """(kind, part): the wires reads(kind) names in runs of BUMP_PART (a gate without wires has the one empty part)."""
    return [(k, p) for k in gm.KINDS for p in range(max(1, -(-len(gm.reads(k)["wires"]) // BUMP_PART)))]


def bump_delta(col):
    """The boundary delta wire column `col` is bumped by in the every-wire test: the members of EDGE but 0, in turn."""
    return ev.EDGE[1 + col % (len(ev.EDGE) - 1)]


def gate_row_circuit(kind):
    """(circuit, row): a row of gate `kind` in the smallest standard circuit that has one."""
    name = {bw.G_NOOP: "tiny_arithmetic", bw.G_CONSTANT: "exponentiation", bw.G_PUBLIC_INPUT: "exponentiation",
            bw.G_BASE_SUM: "tiny_base_sum", bw.G_U32_INTERLEAVE: "u32_bits", bw.G_U32_UNINTERLEAVE: "u32_bits",
            bw.G_ARITHMETIC: "tiny_arithmetic", bw.G_MUL_EXT: "quotient_extension", bw.G_EXPONENTIATION: "exponentiation",
            bw.G_U32_ARITHMETIC: "u32_arithmetic", bw.G_POSEIDON2: "poseidon2", bw.G_ARITH_EXT: "tiny_arithmetic_extension",
            bw.G_POSEIDON: "poseidon", bw.G_RANDOM_ACCESS: "random_access", bw.G_REDUCING: "reducing",
            bw.G_REDUCING_EXT: "reducing_extension", bw.G_COSET_INTERP: "coset_interpolation",
            bw.G_POSEIDON_MDS: "poseidon_mds"}[kind]
    c = circuit(name)
    return c, c.rows_of(kind)[0]


assert set(gm.KINDS) == {k for n in wc.NAMES for k in wc.all_cases()[n].gates} | {bw.G_NOOP, bw.G_CONSTANT, bw.G_PUBLIC_INPUT}


# ---- the identity at zeta, from a proof's openings ----------------------------------------------------------------------------
def zeta_identity(oracle, lay, b, proof, digest):
    """[(Z_H(zeta) sum_k zeta^(n k) q_k(zeta), the model's vanishing sum at zeta)] for the two alphas, in F_p^2, from the
    openings of a flat proof (`lay`: verify_cases.Layout).  The challenger is replayed with oracle.transcript in the
    observation order of k_verify_transcript: circuit digest, public-input hash (no public inputs: four zeros), wires cap ->
    2 betas, 2 gammas; Z cap -> 2 alphas; quotient cap -> zeta."""
    F = gm.Ext
    pr = [int(v) for v in proof]
    ch = [int(v) for v in oracle.transcript([
        (np.concatenate([np.asarray(digest, dtype=np.uint64), np.zeros(4, dtype=np.uint64), proof[lay.wires_cap:lay.zs_cap]]), 4),
        (proof[lay.zs_cap:lay.quotient_cap], 2), (proof[lay.quotient_cap:lay.constants], 2)])]
    betas, gammas, alphas, zeta = ch[0:2], ch[2:4], ch[4:6], (ch[6], ch[7])

    def opened(at, count):
        return [(pr[at + 2 * i], pr[at + 2 * i + 1]) for i in range(count)]

    n, routed = 1 << b["degree_bits"], b["num_routed"]
    np_ = -(-routed // qm.QDF) - 1
    consts = opened(lay.constants, len(b["selectors"]) + 2)
    pps = opened(lay.pps, 2 * np_)
    quot = opened(lay.quotient, 2 * qm.QDF)
    zeta_n = zeta
    for _ in range(b["degree_bits"]):
        zeta_n = F.mul(zeta_n, zeta_n)
    zh = F.sub(zeta_n, F.one)
    l0 = F.mul(zh, wc.e_inv(F.scale(F.sub(zeta, F.one), n)))
    terms = qm.vanishing_terms(b, F, zeta, l0, consts, opened(lay.sigmas, routed), opened(lay.wires, b["num_wires"]),
                               opened(lay.zs, 2), opened(lay.zs_next, 2), [pps[:np_], pps[np_:]], betas, gammas, [F.zero] * 4)
    out = []
    for c in range(2):
        acc = F.zero
        for k in reversed(range(qm.QDF)):
            acc = F.add(F.mul(acc, zeta_n), quot[c * qm.QDF + k])
        out.append((F.mul(zh, acc), qm.fold(F, terms, alphas[c])))
    return out
