// Native plonky3 prover for the Fibonacci AIR (uni-STARK + two-adic FRI PCS + Poseidon2 Merkle MMCS +
// width-12 duplex challenger), producing the per-proof INPUT of the hot path.
//
// The reference cannot produce such proofs (the plonky3 prover lives in an external fork,
// /root/reference/README.md:13-18); it only ships one: artifacts/proof_fibonacci.json.  This prover
// follows the conventions that the reference's in-circuit verifier fixes:
//   transcript          src/p3/challenger.rs:70-169, order src/p3/verifier.rs:135-139, 258, 363-382
//   MMCS hash/compress  src/p3/commit.rs:23-60, paths commit.rs:62-129
//   domains/selectors   src/p3/serde/two_adic.rs:48-147
//   AIR + folding       src/p3/mod.rs:176-221, src/p3/air.rs:63-118, verifier.rs:199-239
//   reduced openings    src/p3/verifier.rs:296-338;  FRI fold  verifier.rs:441-516
//   proof data model    src/p3/serde/proof.rs:16-355 (flattened in `add_virtual_to` order, :357-373)
// Pinned by the artifact: for log_n = 6, 100 queries, 16 PoW bits and the artifact's PoW witness it
// must reproduce all 15,751 field elements of artifacts/proof_fibonacci.json (tests/test_p3_prover.py).
// Host code (data generator for the path's input side); not on the per-proof hot path.
#pragma once
#include <string>
#include <vector>
#include "p3_circuit.h"

namespace p25 {

struct P3ProveParams {
  int log_n = 6;             // trace height 2^log_n (the artifact: 64 rows)
  int log_blowup = 1;        // FriConfig.log_blowup (src/p3/mod.rs:242-246 uses 1); 2 / 3 hold AIRs of degree up to 5 / 9
  int num_queries = 100;
  int pow_bits = 16;
  // proof-of-work witness search starts here (plonky3 grinds with find_any, so any valid witness
  // is a legitimate proof; different witnesses give different query indices = distinct batch items)
  u64 pow_start = 0;
  int threads = 1;
};
// What every plonky3 prover of the library holds of its parameters, host and device: the ranges, the AIR's own checks, and
// a constraint degree that log_blowup's quotient chunks can hold.  Throws std::invalid_argument.
void p3_check_params(const AirProgram& air, int log_n, int log_blowup, int num_queries, int pow_bits);
// The shape of the proof these parameters give for `air` (no checks: a size query answers from it before any)
P3Config p3_config_for(const AirProgram& air, int log_n, int log_blowup, int num_queries, int pow_bits);
// Returns the proof as the flat input vector (add_virtual_to order) and its shape.
std::vector<u64> p3_prove_fibonacci(const P3ProveParams& prm, P3Config& cfg_out);
// Same prover for any AIR given as a program (p3_circuit.h: AirProgram) and its trace, col[c][row];
// constraint degree <= 2^log_blowup + 1 (2^log_quotient_degree quotient chunks; the reference's proof model has one).  Throws
// std::logic_error("quotient identity ...") if the trace does not satisfy the AIR.
std::vector<u64> p3_prove_air(const AirProgram& air, const std::vector<std::vector<u64>>& col, const P3ProveParams& prm,
                              P3Config& cfg_out);
// The same with the proof's public values (air.n_public of them, each < p): observed by the challenger right after the trace
// commitment, read by the AIR's PUBLIC nodes, and appended to the flat vector behind the proof's words (cfg_out.num_inputs()
// + air.n_public words in all).  With no public values the words are p3_prove_air's.
std::vector<u64> p3_prove_air_pv(const AirProgram& air, const std::vector<std::vector<u64>>& col, const std::vector<u64>& pub,
                                 const P3ProveParams& prm, P3Config& cfg_out);
// Preprocessed columns (AirProgram::Preprocessed; include/p25.h "PREPROCESSED COLUMNS") travel in `air.prep`: every prover
// here commits them as it commits the trace, observes the root behind the trace root, opens them at zeta and zeta w_n behind
// the chunk openings and adds a third batch to every query; without columns the words are unchanged.
// The words such a proof has beyond P3Config::num_inputs(): the two openings and every query's row and path.
inline size_t p3_preprocessed_words(int prep_width, int log_n, int log_blowup, int num_queries) {
  return prep_width ? 4 * (size_t)prep_width + (size_t)num_queries * ((size_t)prep_width + 4 * (size_t)(log_n + log_blowup)) : 0;
}
// Auxiliary columns (AirProgram::Aux; include/p25.h "AUXILIARY COLUMNS") travel in `air.aux`: every prover here samples the
// challenges behind the public values, builds the running sums, commits them as 2 AW base columns, observes that root and
// only then samples alpha; it opens them behind the preprocessed openings and adds a last batch to every query.  A zero
// denominator throws std::invalid_argument naming column and row.  Without such columns the words are unchanged.
// The words such a proof has beyond P3Config::num_inputs(): the root, the two openings and every query's row and path.
inline size_t p3_aux_words(int aux_width, int log_n, int log_blowup, int num_queries) {
  return aux_width ? 4 + 8 * (size_t)aux_width + (size_t)num_queries * (2 * (size_t)aux_width + 4 * (size_t)(log_n + log_blowup)) : 0;
}
// Checking a trace (include/p25.h "CHECKING A TRACE"; p3_check.cpp): the report -- p3ck_words(AW, constraints) words,
// p3_check_lanes.h -- of `col` against `air`, by the per-row functions the device runs.  No proof is made: log_blowup is
// needed only because the challenges of an AIR with auxiliary columns hang on the trace's commitment.  Throws
// std::invalid_argument as p3_prove_air_pv does for its arguments.
std::vector<u64> p3_check_air(const AirProgram& air, const std::vector<std::vector<u64>>& col, const std::vector<u64>& pub,
                              int log_n, int log_blowup, int threads);
// The challenges the proof of this trace would draw: the transcript is the trace root, the preprocessed root if the AIR
// has such columns, the public values; then air.aux.n_challenges samples.
std::vector<gl::E2> p3_trace_challenges(const AirProgram& air, const std::vector<std::vector<u64>>& col, const std::vector<u64>& pub,
                                        int log_n, int log_blowup, int threads);
// The commitment of a preprocessed matrix: the Poseidon2 MMCS root over the columns' LDE on 7 H_{n 2^log_blowup} in
// bit-reversed leaf order, the commit the trace gets.  Throws std::invalid_argument (width 0 included: nothing to commit).
std::array<u64, 4> p3_preprocessed_commit(const AirProgram::Preprocessed& prep, int log_blowup, int threads);
// A periodic column on the quotient coset 7 H_{n Q}, Q = 2^lqd (AirProgram::Periodic; include/p25.h "PERIODIC COLUMNS"):
// T[r] = q(7^(n/P) u^r), u = w_{n Q}^(n/P) of order P Q, for r < P Q -- the coset LDE of the interpolant q whose P
// coefficients are `coef`.  The column's value at the point of natural index j, x_j = 7 w_{n Q}^j, is T[j mod (P Q)].
std::vector<u64> p3_periodic_table(const std::vector<u64>& coef, int log_n, int lqd);
// serde-JSON text in the reference's format (proof.rs:16-19: field elements are {"value": u64})
std::string p3_inputs_to_json(const std::vector<u64>& inputs, const P3Config& cfg);

}  // namespace p25
