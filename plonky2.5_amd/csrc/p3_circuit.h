// The plonky3-verifier circuit: host-side restatement of /root/reference/src/p3 (mod.rs, verifier.rs,
// challenger.rs, commit.rs, extension.rs, air.rs, serde/{proof,two_adic}.rs).  Emits the same gates in
// the same order through the CircuitBuilder of builder.h.  Runs once per circuit shape.
#pragma once
#include <string>
#include <vector>
#include "builder.h"

namespace p25 {

// src/p3/serde/fri.rs:3-8
struct P3FriConfig {
  int log_blowup = 1;
  int num_queries = 100;
  int proof_of_work_bits = 16;
};
// src/p3/serde/proof.rs:401-410; derived from the proof's shape at src/p3/mod.rs:74-87
struct P3Config {
  P3FriConfig fri_config;
  int log_quotient_degree = 0;
  int log_trace_height = 6;
  int trace_width = 3;
  int opening_matrix_log_max_height = 7;
  int opening_proof_query_openings_opened_values_length = 2;
  int degree_bits = 6;
  // number of field elements of one proof in `add_virtual_to` order
  size_t num_inputs() const;
};

// Proof<Target> (src/p3/serde/proof.rs:349-383)
struct P3CommitPhaseStep {
  Ext sibling_value;
  std::vector<std::array<Target, 4>> opening_proof;
};
struct P3BatchOpening {
  std::vector<std::vector<Target>> opened_values;
  std::vector<std::array<Target, 4>> opening_proof;
};
struct P3ProofTarget {
  std::array<Target, 4> trace_commit, quotient_commit;
  std::vector<Ext> trace_local, trace_next;
  std::vector<std::vector<Ext>> quotient_chunks;
  std::vector<std::array<Target, 4>> commit_phase_commits;
  std::vector<std::vector<P3CommitPhaseStep>> query_proofs;
  Ext final_poly;
  Target pow_witness;
  // this library's extension (AirProgram::PREP_LOCAL / PREP_NEXT): the preprocessed columns at zeta and zeta w_n; empty
  // for an AIR without preprocessed columns
  std::vector<Ext> prep_local, prep_next;
  // this library's extension (AirProgram::AUX_LOCAL / AUX_NEXT): the commitment of the auxiliary (second-phase) matrix and
  // its 2 AW base columns at zeta and zeta w_n, behind the preprocessed openings; empty for an AIR without auxiliary columns
  std::array<Target, 4> aux_commit{};
  std::vector<Ext> aux_local, aux_next;
  // per query: the trace batch, the quotient batch, for an AIR with preprocessed columns the preprocessed batch and, for an
  // AIR with auxiliary columns, the auxiliary batch -- up to four, in this order
  std::vector<std::vector<P3BatchOpening>> query_openings;
  int degree_bits;
};

// src/p3/air.rs:20-27
struct VerifierConstraintFolder {
  std::vector<Ext> trace_local, trace_next;
  std::vector<Ext> public_values;   // this library's extension (AirProgram::PUBLIC): base elements embedded in the extension
  std::vector<Ext> periodic;        // this library's extension (AirProgram::PERIODIC): the periodic columns at zeta, by column
  std::vector<Ext> prep_local, prep_next;   // this library's extension (AirProgram::PREP_LOCAL / PREP_NEXT): the opened values
  // this library's extension (AirProgram::CHALLENGE / AUX_LOCAL / AUX_NEXT): the sampled challenges and the auxiliary
  // columns at zeta and zeta w_n, each recomposed from its two opened component columns
  std::vector<Ext> challenges, aux_local, aux_next;
  Ext is_first_row, is_last_row, is_transition, alpha, accumulator;
  // air.rs:69-88, 90-118
  void assert_zero(CircuitBuilder& cb, Ext x);
  void assert_eq(CircuitBuilder& cb, Ext x, Ext y);
  void when_assert_eq(CircuitBuilder& cb, Ext condition, Ext x, Ext y);
};
// src/p3/air.rs:10-18 (the plugin interface a user implements per inner STARK)
struct Air {
  virtual ~Air() {}
  virtual std::string name() const = 0;
  virtual int width() const = 0;
  // public values of a proof (uni-stark's `public_values`); the reference's trait has none
  virtual int n_public() const { return 0; }
  // the AIR's periodic columns at zeta, in column order (this library's extension; the reference's trait has none): emits
  // the gates that compute them and throws std::invalid_argument for a period above the trace height 2^log_n
  virtual std::vector<Ext> periodic_at(CircuitBuilder&, const Ext& /*zeta*/, int /*log_n*/) const { return {}; }
  // the preprocessed columns (this library's extension; the reference's trait has none): their count, and the 4 words of
  // their commitment for a trace of 2^log_n rows under this log_blowup -- verifying-key data the circuit holds as constants
  virtual int preprocessed_width() const { return 0; }
  virtual std::array<u64, 4> preprocessed_commit(int /*log_n*/, int /*log_blowup*/) const { return {}; }
  // the auxiliary (challenge-phase) columns (this library's extension; the reference's trait has none): the challenges
  // sampled behind the public values and the F_p^2 columns committed behind them
  virtual int n_challenges() const { return 0; }
  virtual int aux_width() const { return 0; }
  virtual void eval(VerifierConstraintFolder& folder, CircuitBuilder& cb) const = 0;
};
// src/p3/mod.rs:160-221 (the test's FibonacciAir)
struct FibonacciAir : Air {
  std::string name() const override { return "Fibonacci"; }
  int width() const override { return 3; }
  void eval(VerifierConstraintFolder& folder, CircuitBuilder& cb) const override;
};

// An AIR as data: the reference's plugin interface is a Rust trait whose `eval` is code
// (air.rs:10-18); across a C ABI the same information travels as an expression DAG.  Nodes refer to
// earlier nodes; a constraint is a node that must vanish on the rows selected by `when`, folded in
// order exactly as VerifierConstraintFolder does (air.rs:69-118): `always` -> assert_zero(node),
// otherwise assert_zero(selector * node).  Used by BOTH sides of the path's input: the in-circuit
// verifier (ProgramAir below) and the native plonky3 prover (p3_prover.h).
struct AirProgram {
  // PUBLIC(a): public value a < n_public of the proof (uni-stark's `builder.public_values()[a]`): degree 0 like CONST
  // PERIODIC(a): periodic column a at the current row (this library's extension, like PUBLIC; include/p25.h "PERIODIC
  // COLUMNS"): degree 1 like LOCAL
  // PREP_LOCAL(a) / PREP_NEXT(a): preprocessed column a at the current / the next row, cyclic as NEXT is (this library's
  // extension; include/p25.h "PREPROCESSED COLUMNS"): degree 1 like LOCAL
  // CHALLENGE(a): challenge a < aux.n_challenges, an element of F_p^2 sampled after the trace is committed: degree 0
  // AUX_LOCAL(a) / AUX_NEXT(a): auxiliary column a < aux.width() at the current / the next row, cyclic as NEXT is (this
  // library's extension; include/p25.h "AUXILIARY COLUMNS"): values in F_p^2, degree 1 like LOCAL.  An AIR with any of
  // the three is evaluated in F_p^2 throughout.
  enum Op : uint32_t { LOCAL = 0, NEXT = 1, CONST = 2, ADD = 3, SUB = 4, MUL = 5, PUBLIC = 6, PERIODIC = 7, PREP_LOCAL = 8,
                       PREP_NEXT = 9, CHALLENGE = 10, AUX_LOCAL = 11, AUX_NEXT = 12 };
  static constexpr int MAX_CHALLENGES = 8, MAX_AUX = 16;   // P25_AIR_MAX_CHALLENGES, P25_AIR_MAX_AUX
  static constexpr int MAX_PREPROCESSED = 64;   // P25_AIR_MAX_PREPROCESSED
  static constexpr int MAX_PUBLIC = 64;   // P25_AIR_MAX_PUBLIC
  static constexpr int MAX_PERIODIC = 32, MAX_LOG_PERIOD = 8;   // P25_AIR_MAX_PERIODIC, P25_AIR_MAX_LOG_PERIOD
  enum When : uint32_t { ALWAYS = 0, FIRST_ROW = 1, LAST_ROW = 2, TRANSITION = 3 };
  struct Node {
    uint32_t op, a, b;  // LOCAL/NEXT: a = column; PUBLIC: a = index; PERIODIC: a = periodic column; PREP_LOCAL/PREP_NEXT: a = preprocessed column; CHALLENGE: a = challenge; AUX_LOCAL/AUX_NEXT: a = auxiliary column; ADD/SUB/MUL: a, b = earlier node indices
    u64 value;          // CONST
  };
  struct Constraint {
    uint32_t node, when;
  };
  int width = 0;
  int n_public = 0;
  // A periodic column is part of the AIR like a constant: on trace row i it is values[i mod P], P = 2^log_period, and as a
  // polynomial over the trace domain q(x^(n/P)), q the interpolant of `values` over <w_P>.  Neither committed nor opened.
  struct Periodic {
    uint32_t log_period;       // 1..MAX_LOG_PERIOD, and at most the trace's log height (check_periodic)
    std::vector<u64> values;   // [2^log_period], each < p
  };
  std::vector<Periodic> periodic;
  // The preprocessed trace: a matrix of known columns as high as the trace, committed once like the trace (the commitment is
  // verifying-key data, p3_preprocessed_commit in p3_prover.h), opened at zeta and zeta w_n and queried like the trace.
  struct Preprocessed {
    uint32_t width = 0;        // 0..MAX_PREPROCESSED
    uint32_t log_n = 0;        // the trace's log height (check_preprocessed)
    std::vector<u64> values;   // [2^log_n][width], row-major like a trace, each < p
  };
  Preprocessed prep;
  // The auxiliary (second-phase) trace: column j is the running sum over the rows of num_j / den_j in F_p^2, S_j(0) = 0,
  // S_j(i + 1) = S_j(i) + num_j(i) / den_j(i), the two nodes evaluated on trace row i with the challenges at hand.  The
  // prover builds it after sampling the challenges and commits it as 2 width() base columns (column j's components at 2 j
  // and 2 j + 1); the constraints over it are the AIR's own.  num and den read neither AUX_LOCAL nor AUX_NEXT.
  struct AuxColumn {
    uint32_t num, den;   // node indices
  };
  struct Aux {
    uint32_t n_challenges = 0;        // 0..MAX_CHALLENGES
    std::vector<AuxColumn> columns;   // 0..MAX_AUX
    uint32_t width() const { return (uint32_t)columns.size(); }
  };
  Aux aux;
  // whether any node is a CHALLENGE, AUX_LOCAL or AUX_NEXT: such an AIR is evaluated in F_p^2 throughout
  bool reads_aux() const {
    for (const Node& nd : nodes)
      if (nd.op >= CHALLENGE && nd.op <= AUX_NEXT) return true;
    return false;
  }
  std::vector<Node> nodes;
  std::vector<Constraint> constraints;
  // throws std::invalid_argument on malformed programs (a PUBLIC index >= n_public, n_public > MAX_PUBLIC, a PERIODIC index
  // past the columns, more than MAX_PERIODIC columns, a log_period outside 1..MAX_LOG_PERIOD, a value >= p among them)
  // and on constraint degree > 9 (selector included; eight quotient chunks).  The reference's proof model carries exactly one chunk (serde/proof.rs:41-48, degree <= 2); more chunks are this
  // library's extension of it, and log_quotient_degree() of them must not exceed the FRI log_blowup (checked by the callers).
  void validate() const;
  // the one check that needs the trace height: throws std::invalid_argument for a column with log_period > log_n
  void check_periodic(int log_n) const;
  // the same for the preprocessed matrix: throws std::invalid_argument if it has columns and its log_n is not the trace's
  void check_preprocessed(int log_n) const;
  // coefficients of column c's interpolant q (degree < P, q(w_P^j) = values[j]): what the evaluation at zeta and the
  // table on the quotient coset (p3_periodic_table, p3_prover.h) start from
  std::vector<u64> periodic_coefficients(size_t c) const;
  // the degree of every node in one pass over the DAG, saturating at DEGREE_SAT (a chain of squarings overflows any integer)
  static constexpr int DEGREE_SAT = 1 << 16;
  std::vector<int> node_degrees() const;
  int node_degree(uint32_t i) const { return node_degrees()[i]; }
  // max over the constraints of their degree with the selector's counted, and uni-stark's get_log_quotient_degree of it:
  // log2_ceil(max(degree, 2) - 1) -- 0 for degree <= 2, 1 for 3, 2 for 4..5, 3 for 6..9
  int max_constraint_degree() const;
  int log_quotient_degree() const;
  // the test AIR of src/p3/mod.rs:176-221 in this form (same constraints, same order)
  static AirProgram fibonacci();

  // Generic evaluation, nodes computed on demand in constraint order (so that the circuit form emits
  // its gates in the order the reference's hand-written `eval` does).  ops: cst(u64), pub(index), per(column),
  // prep_local(column), prep_next(column), challenge(index), aux_local(column), aux_next(column), add, sub, mul.
  template <class T, class Ops, class Emit>
  void fold(const std::vector<T>& local, const std::vector<T>& next, const T sel[4], Ops& ops, Emit&& emit) const {
    NodeValues<T> nv(nodes.size());
    for (const Constraint& c : constraints) {
      const T& v = node_value(c.node, nv, local, next, ops);
      emit(c.when == ALWAYS ? v : ops.mul(sel[c.when], v));
    }
  }
  // The auxiliary columns' terms on one row: emit(column, num_j, den_j) in column order, nodes computed on demand in that
  // order and shared between the columns.
  template <class T, class Ops, class Emit>
  void fold_aux(const std::vector<T>& local, const std::vector<T>& next, Ops& ops, Emit&& emit) const {
    NodeValues<T> nv(nodes.size());
    for (size_t j = 0; j < aux.columns.size(); j++) {
      const T num = node_value(aux.columns[j].num, nv, local, next, ops);
      const T den = node_value(aux.columns[j].den, nv, local, next, ops);
      emit(j, num, den);
    }
  }

 private:
  template <class T>
  struct NodeValues {
    std::vector<T> val;
    std::vector<char> have;
    explicit NodeValues(size_t n) : val(n), have(n, 0) {}
  };
  // iterative post-order evaluation of the sub-DAG under `root`
  template <class T, class Ops>
  const T& node_value(uint32_t root, NodeValues<T>& nv, const std::vector<T>& local, const std::vector<T>& next, Ops& ops) const {
    std::vector<T>& val = nv.val;
    std::vector<char>& have = nv.have;
    std::vector<uint32_t> stack{root};
    while (!stack.empty()) {
      uint32_t i = stack.back();
      if (have[i]) {
        stack.pop_back();
        continue;
      }
      const Node& nd = nodes[i];
      if (nd.op == LOCAL) {
        val[i] = local[nd.a];
      } else if (nd.op == NEXT) {
        val[i] = next[nd.a];
      } else if (nd.op == CONST) {
        val[i] = ops.cst(nd.value);
      } else if (nd.op == PUBLIC) {
        val[i] = ops.pub(nd.a);
      } else if (nd.op == PERIODIC) {
        val[i] = ops.per(nd.a);
      } else if (nd.op == PREP_LOCAL) {
        val[i] = ops.prep_local(nd.a);
      } else if (nd.op == PREP_NEXT) {
        val[i] = ops.prep_next(nd.a);
      } else if (nd.op == CHALLENGE) {
        val[i] = ops.challenge(nd.a);
      } else if (nd.op == AUX_LOCAL) {
        val[i] = ops.aux_local(nd.a);
      } else if (nd.op == AUX_NEXT) {
        val[i] = ops.aux_next(nd.a);
      } else {
        if (!have[nd.a]) {
          stack.push_back(nd.a);
          continue;
        }
        if (!have[nd.b]) {
          stack.push_back(nd.b);
          continue;
        }
        val[i] = nd.op == ADD ? ops.add(val[nd.a], val[nd.b]) : nd.op == SUB ? ops.sub(val[nd.a], val[nd.b]) : ops.mul(val[nd.a], val[nd.b]);
      }
      have[i] = 1;
      stack.pop_back();
    }
    return val[root];
  }
};
struct ProgramAir : Air {
  AirProgram prog;
  explicit ProgramAir(AirProgram p) : prog(std::move(p)) { prog.validate(); }
  std::string name() const override { return "Program"; }
  int width() const override { return prog.width; }
  int n_public() const override { return prog.n_public; }
  // emission order: p3_circuit.cpp
  std::vector<Ext> periodic_at(CircuitBuilder& cb, const Ext& zeta, int log_n) const override;
  int preprocessed_width() const override { return (int)prog.prep.width; }
  std::array<u64, 4> preprocessed_commit(int log_n, int log_blowup) const override;   // p3_prover.cpp
  int n_challenges() const override { return (int)prog.aux.n_challenges; }
  int aux_width() const override { return (int)prog.aux.width(); }
  void eval(VerifierConstraintFolder& folder, CircuitBuilder& cb) const override;
};

// CircuitBuilderP3Arithmetic::p3_verify_proof (src/p3/mod.rs:66-94).  Registers the proof's virtual
// targets as the circuit's per-proof inputs (cb.input_targets, `add_virtual_to` order).  An AIR with public values adds
// air.n_public() input targets behind the proof's, observes them after the trace commitment (where uni-stark's verifier has
// `challenger.observe_slice(public_values)`) and registers them as the circuit's public inputs, in order.  An AIR with
// preprocessed columns adds their openings and a third batch per query to the proof's targets (include/p25.h "PREPROCESSED
// COLUMNS" has the positions), holds their commitment as four constants, observes it directly after the trace commitment
// and hands the opening proof a third (commitment, matrices, points) entry; without such columns the circuit is as it was.
// An AIR with auxiliary columns (include/p25.h "AUXILIARY COLUMNS") samples its challenges behind the public values, then
// observes the auxiliary commitment -- a proof target, not a constant -- before alpha, and hands the opening proof one more
// entry, the last; without such columns the circuit is as it was.
P3ProofTarget p3_verify_proof(CircuitBuilder& cb, const P3Config& config, const Air& air);

// gadget-level entry points (src/p3/mod.rs:40-45, 96-147), exposed for the gadget tests
Target p3_constant(CircuitBuilder& cb, u64 v);
Target p3_and(CircuitBuilder& cb, Target x, Target y);
Target p3_xor(CircuitBuilder& cb, Target x, Target y);
Target p3_lsh(CircuitBuilder& cb, Target x, int n);
Target p3_rsh(CircuitBuilder& cb, Target x, int n);
Target reverse_p3(CircuitBuilder& cb, Target x);
Target reverse_p3_bits_len(CircuitBuilder& cb, Target x, int bit_len);


// Small circuits mirroring the reference's gadget tests (src/p3/mod.rs:271-494: test_p3_and / xor /
// lsh / rsh / reverse; src/p3/commit.rs:173-198: test_compress).  Inputs are virtual targets
// [operands..., expected...]; the gadget's result is connected to `expected`, so a wrong expectation
// surfaces as a witness conflict exactly like a failing `connect` upstream.
enum GadgetKind { GADGET_AND = 0, GADGET_XOR, GADGET_LSH, GADGET_RSH, GADGET_REVERSE, GADGET_COMPRESS, GADGET_EXP, GADGET_HASH_SLICES,
                  GADGET_CONNECTED_INPUTS, GADGET_EXT_ARITH, GADGET_POSEIDON_MERKLE, GADGET_PUBLIC_INPUTS,
                  GADGET_INTERLEAVE_U32, GADGET_UNINTERLEAVE_TO_U32, GADGET_REFERENCE_GATES };
Circuit build_gadget_circuit(int kind, int param, const CircuitConfig& cfg = CircuitConfig());

}  // namespace p25
