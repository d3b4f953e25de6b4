// tests/native/p3_verify_lanes.cpp for AIRs with challenges and auxiliary columns (include/p25.h "AUXILIARY COLUMNS"): the
// transcript, identity, fold, Merkle and verdict lanes of a batch in plain loops.
//   p3_verify_lanes_aux <data>   data (u64 words) = width | n_nodes | n_constraints | log_n | log_blowup | num_queries |
//                                pow_bits | n_proofs | n_challenges | aux width | nodes[n_nodes][op, a, b, value] |
//                                constraints[n_constraints][node, when] | columns[aux width][num, den] | proofs[n_proofs][num_inputs]
//   p3_verify_lanes_aux <data> full   the whole AIR form: four more head words n_public | n_periodic | prep width | 0, and
//                                between the columns and the proofs periodic[n_periodic]{log_period, values[2^log_period]} |
//                                prep[2^log_n][prep width] | prep_root[4] (the verifying key's commitment; present only with
//                                prep width > 0); a proof's num_inputs words end in its n_public public values
// prints one verdict per proof.  Linked against libp25.so for the AIR's compilation and the shape only.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <vector>
#include "p3_verify_lanes.h"

using namespace p25;

int main(int argc, char** argv) {
  if (argc != 2 && !(argc == 3 && !strcmp(argv[2], "full"))) return 2;
  const bool full = argc == 3;
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
  const size_t head_words = full ? 14 : 10;
  if (w.size() < head_words) return 2;
  AirProgram air;
  air.width = (int)w[0];
  const size_t n_nodes = w[1], n_cons = w[2], n_proofs = w[7], aw = w[9];
  const size_t n_public = full ? w[10] : 0, n_per = full ? w[11] : 0, pw = full ? w[12] : 0;
  air.aux.n_challenges = (uint32_t)w[8];
  air.n_public = (int)n_public;
  size_t at = head_words;
  auto need = [&](size_t words) {
    if (at + words > w.size()) {
      fprintf(stderr, "data file too short\n");
      exit(2);
    }
  };
  need(4 * n_nodes + 2 * n_cons + 2 * aw);
  for (size_t i = 0; i < n_nodes; i++, at += 4)
    air.nodes.push_back(AirProgram::Node{(uint32_t)w[at], (uint32_t)w[at + 1], (uint32_t)w[at + 2], w[at + 3]});
  for (size_t i = 0; i < n_cons; i++, at += 2) air.constraints.push_back(AirProgram::Constraint{(uint32_t)w[at], (uint32_t)w[at + 1]});
  for (size_t i = 0; i < aw; i++, at += 2) air.aux.columns.push_back(AirProgram::AuxColumn{(uint32_t)w[at], (uint32_t)w[at + 1]});
  for (size_t c = 0; c < n_per; c++) {
    need(1);
    AirProgram::Periodic pc;
    pc.log_period = (uint32_t)w[at++];
    if (pc.log_period > AirProgram::MAX_LOG_PERIOD) return 2;
    need((size_t)1 << pc.log_period);
    pc.values.assign(w.begin() + at, w.begin() + at + ((size_t)1 << pc.log_period));
    at += pc.values.size();
    air.periodic.push_back(pc);
  }
  u64 prep_root[4] = {0, 0, 0, 0};
  if (pw) {
    if (w[3] > 24) return 2;
    const size_t rows = (size_t)1 << w[3];
    need(pw * rows + 4);
    air.prep.width = (uint32_t)pw;
    air.prep.log_n = (uint32_t)w[3];
    air.prep.values.assign(w.begin() + at, w.begin() + at + pw * rows);
    at += pw * rows;
    for (int i = 0; i < 4; i++) prep_root[i] = w[at++];
  }
  const P3ProverDev dev(air, (int)w[3], (int)w[4], (int)w[5], (int)w[6]);
  P3VerifyArgs a = dev.verify_args();
  if (w.size() != at + n_proofs * (size_t)a.num_inputs) {
    fprintf(stderr, "data file has the wrong size\n");
    return 2;
  }
  a.proofs = w.data() + at;
  a.stride = a.num_inputs;
  a.n_proofs = (uint32_t)n_proofs;
  if (pw) a.prep_root = prep_root;
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
