// tests/native/p3_verify_lanes.cpp for AIRs with challenges and auxiliary columns (include/p25.h "AUXILIARY COLUMNS"): the
// transcript, identity, fold, Merkle and verdict lanes of a batch in plain loops.
//   p3_verify_lanes_aux <data>   data (u64 words) = width | n_nodes | n_constraints | log_n | log_blowup | num_queries |
//                                pow_bits | n_proofs | n_challenges | aux width | nodes[n_nodes][op, a, b, value] |
//                                constraints[n_constraints][node, when] | columns[aux width][num, den] | proofs[n_proofs][num_inputs]
// prints one verdict per proof.  Linked against libp25.so for the AIR's compilation and the shape only.
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "p3_verify_lanes.h"

using namespace p25;

int main(int argc, char** argv) {
  if (argc != 2) return 2;
  FILE* f = fopen(argv[1], "rb");
  if (!f) {
    fprintf(stderr, "cannot open %s\n", argv[1]);
    return 2;
  }
  std::vector<u64> w;
  u64 buf[1 << 13];
  size_t n;
  while ((n = fread(buf, 8, 1 << 13, f)) > 0) w.insert(w.end(), buf, buf + n);
  fclose(f);
  if (w.size() < 10) return 2;
  AirProgram air;
  air.width = (int)w[0];
  const size_t n_nodes = w[1], n_cons = w[2], n_proofs = w[7], aw = w[9];
  air.aux.n_challenges = (uint32_t)w[8];
  const size_t head = 10 + 4 * n_nodes + 2 * n_cons + 2 * aw;
  if (w.size() < head) return 2;
  const u64* p = w.data() + 10;
  for (size_t i = 0; i < n_nodes; i++, p += 4) air.nodes.push_back(AirProgram::Node{(uint32_t)p[0], (uint32_t)p[1], (uint32_t)p[2], p[3]});
  for (size_t i = 0; i < n_cons; i++, p += 2) air.constraints.push_back(AirProgram::Constraint{(uint32_t)p[0], (uint32_t)p[1]});
  for (size_t i = 0; i < aw; i++, p += 2) air.aux.columns.push_back(AirProgram::AuxColumn{(uint32_t)p[0], (uint32_t)p[1]});
  const P3ProverDev dev(air, (int)w[3], (int)w[4], (int)w[5], (int)w[6]);
  P3VerifyArgs a = dev.verify_args();
  if (w.size() != head + n_proofs * (size_t)a.num_inputs) {
    fprintf(stderr, "data file has the wrong size\n");
    return 2;
  }
  a.proofs = p;
  a.stride = a.num_inputs;
  a.n_proofs = (uint32_t)n_proofs;
  std::vector<u64> chal(n_proofs * a.chal_stride), folded(n_proofs * a.num_queries * a.k * 2);
  std::vector<uint32_t> status(n_proofs);
  a.chal = chal.data();
  a.folded = folded.data();
  a.status = status.data();
  for (uint32_t i = 0; i < a.n_proofs; i++) {
    uint32_t key = p3vlane::transcript_lane(a, i);
    auto merge = [&](uint32_t k) {
      if (k < key) key = k;
    };
    // every lane runs, in an order that is NOT the verifier's: the minimum must still be its first failure
    if (!p3vlane::identity_lane(a, i)) merge(p3v_key_constraints(a));
    for (uint32_t q = a.num_queries; q-- > 0;) merge(p3vlane::fold_lane(a, i, q));
    for (uint32_t t = a.nb + a.k; t-- > 0;)
      for (uint32_t q = a.num_queries; q-- > 0;) merge(p3vlane::merkle_lane(a, t, i, q));
    printf("%u\n", p3vlane::verdict_lane(a, key));
  }
  return 0;
}
