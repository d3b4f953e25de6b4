// Host side of the device plonky3 prover: the AIR's register program, the shape tables and the launch sequence of one
// group of proofs, which mirrors p3_prove_air (p3_prover.cpp) stage by stage.  The kernels are in kernels_p3.hip.
#include <algorithm>
#include <functional>
#include "p3_check_lanes.h"
#include "p3_prover.h"
#include "p3_prover_impl.h"
#include "staging.h"

namespace p25 {

// ---------------------------------------------------------------------------------------------------------------------
// AirProgram -> register program.  Nodes are visited in the order AirProgram::fold evaluates them; a LOCAL / NEXT / CONST /
// PUBLIC / PERIODIC / PREP_LOCAL / PREP_NEXT / CHALLENGE / AUX_LOCAL / AUX_NEXT node becomes an operand, an arithmetic node takes a slot from its evaluation to its last use.
// ---------------------------------------------------------------------------------------------------------------------
namespace {
struct P3Root {
  uint32_t node, tag;   // tag: what the EMIT carries in `dst` -- a constraint's `when`, an auxiliary term's output index
};
// one register program emitting `roots` in order; CONST operands are appended to `consts`
std::vector<P3Instr> compile_roots(const AirProgram& air, const std::vector<P3Root>& roots, std::vector<u64>& consts,
                                   uint32_t& max_live) {
  typedef AirProgram A;
  const size_t N = air.nodes.size();
  std::vector<P3Instr> instr;
  auto is_leaf = [&](uint32_t i) { return air.nodes[i].op <= A::CONST || air.nodes[i].op >= A::PUBLIC; };
  // uses of every arithmetic node by the nodes and constraints that are evaluated
  std::vector<uint32_t> uses(N, 0);
  std::vector<char> seen(N, 0);
  std::function<void(uint32_t)> count = [&](uint32_t root) {
    std::vector<uint32_t> stack{root};
    while (!stack.empty()) {
      const uint32_t i = stack.back();
      stack.pop_back();
      if (seen[i]) continue;
      seen[i] = 1;
      if (is_leaf(i)) continue;
      uses[air.nodes[i].a]++;
      uses[air.nodes[i].b]++;
      stack.push_back(air.nodes[i].a);
      stack.push_back(air.nodes[i].b);
    }
  };
  for (const auto& c : roots) {
    uses[c.node]++;
    count(c.node);
  }
  std::vector<uint32_t> const_index(N, 0), slot_of(N, 0), free_slots;
  std::vector<char> have(N, 0);
  uint32_t n_slots = 0, live = 0;
  auto operand = [&](uint32_t i) -> uint32_t {
    const A::Node& nd = air.nodes[i];
    if (nd.op == A::LOCAL) return (P3_OPND_LOCAL << 28) | nd.a;
    if (nd.op == A::NEXT) return (P3_OPND_NEXT << 28) | nd.a;
    if (nd.op == A::PUBLIC) return (P3_OPND_PUBLIC << 28) | nd.a;
    if (nd.op == A::PREP_LOCAL) return (P3_OPND_PREP_LOCAL << 28) | nd.a;
    if (nd.op == A::PREP_NEXT) return (P3_OPND_PREP_NEXT << 28) | nd.a;
    if (nd.op == A::CHALLENGE) return (P3_OPND_CHALLENGE << 28) | nd.a;
    if (nd.op == A::AUX_LOCAL) return (P3_OPND_AUX_LOCAL << 28) | nd.a;
    if (nd.op == A::AUX_NEXT) return (P3_OPND_AUX_NEXT << 28) | nd.a;
    if (nd.op == A::PERIODIC) {
      uint32_t off = 0;   // words of the columns before it
      for (uint32_t c = 0; c < nd.a; c++) off += 1u << air.periodic[c].log_period;
      return (P3_OPND_PERIODIC << 28) | (air.periodic[nd.a].log_period << 24) | off;
    }
    if (nd.op == A::CONST) {
      if (!have[i]) {
        have[i] = 1;
        const_index[i] = (uint32_t)consts.size();
        consts.push_back(nd.value);
      }
      return (P3_OPND_CONST << 28) | const_index[i];
    }
    return (P3_OPND_SLOT << 28) | slot_of[i];
  };
  auto release = [&](uint32_t i) {
    if (is_leaf(i)) return;
    if (--uses[i] == 0) {
      free_slots.push_back(slot_of[i]);
      live--;
    }
  };
  for (const auto& c : roots) {
    std::vector<uint32_t> stack{c.node};
    while (!stack.empty()) {
      const uint32_t i = stack.back();
      if (is_leaf(i) || have[i]) {
        stack.pop_back();
        continue;
      }
      const A::Node& nd = air.nodes[i];
      if (!is_leaf(nd.a) && !have[nd.a]) {
        stack.push_back(nd.a);
        continue;
      }
      if (!is_leaf(nd.b) && !have[nd.b]) {
        stack.push_back(nd.b);
        continue;
      }
      P3Instr in{nd.op, 0, operand(nd.a), operand(nd.b)};
      release(nd.a);
      release(nd.b);
      if (free_slots.empty()) free_slots.push_back(n_slots++);
      in.dst = slot_of[i] = free_slots.back();
      free_slots.pop_back();
      live++;
      max_live = std::max(max_live, live);
      instr.push_back(in);
      have[i] = 1;
      stack.pop_back();
    }
    instr.push_back(P3Instr{P3_OP_EMIT, c.tag, operand(c.node), 0});
    release(c.node);
  }
  if (n_slots > P3_MAX_LIVE)
    throw std::invalid_argument("p25_p3_prover_create: the AIR keeps " + std::to_string(n_slots) +
                                " intermediate values alive at once; the device form holds at most " + std::to_string(P3_MAX_LIVE));
  if (instr.size() > P3_MAX_INSTR || consts.size() >= (1u << 28))
    throw std::invalid_argument("p25_p3_prover_create: the AIR compiles to more than " + std::to_string(P3_MAX_INSTR) +
                                " instructions, the device form's limit");
  return instr;
}
}  // namespace

P3AirDevice P3AirDevice::compile(const AirProgram& air) {
  P3AirDevice out;
  std::vector<P3Root> roots;
  for (const auto& c : air.constraints) roots.push_back(P3Root{c.node, c.when});
  out.instr = compile_roots(air, roots, out.consts, out.max_live);
  if (air.aux.width()) {   // the auxiliary columns' terms: num_0, den_0, num_1, den_1, ...
    roots.clear();
    for (uint32_t j = 0; j < air.aux.width(); j++) {
      roots.push_back(P3Root{air.aux.columns[j].num, 2 * j});
      roots.push_back(P3Root{air.aux.columns[j].den, 2 * j + 1});
    }
    out.aux_instr = compile_roots(air, roots, out.consts, out.max_live);
  }
  if (out.consts.empty()) out.consts.push_back(0);
  return out;
}

// ---------------------------------------------------------------------------------------------------------------------
P3ProverDev::P3ProverDev(const AirProgram& air, int log_n, int log_blowup, int num_queries, int pow_bits) {
  p3_check_params(air, log_n, log_blowup, num_queries, pow_bits);
  if (num_queries > 65535) throw std::invalid_argument("p25_p3_prover_create: more than 65535 queries (the gather's grid limit)");
  prog_ = P3AirDevice::compile(air);
  cfg_ = p3_config_for(air, log_n, log_blowup, num_queries, pow_bits);
  const int k = log_n, B = log_blowup, L = k + B, W = air.width, lqd = cfg_.log_quotient_degree;
  const size_t n = (size_t)1 << k, Q = (size_t)1 << lqd;

  P3Shape& s = shape_;
  s = P3Shape{};
  s.k = k; s.B = B; s.L = L; s.lqd = lqd; s.Q = (uint32_t)Q; s.W = W;
  s.num_queries = num_queries; s.pow_bits = pow_bits;
  s.n_instr = (uint32_t)prog_.instr.size();
  s.n_public = (uint32_t)air.n_public;
  n_constraints_ = (uint32_t)air.constraints.size();
  for (const auto& pc : air.periodic) per_values_.insert(per_values_.end(), pc.values.begin(), pc.values.end());
  s.PW = air.prep.width;
  if (s.PW) prep_values_ = air.prep.values;
  const uint32_t PW = s.PW;
  s.NC = air.aux.n_challenges;
  s.AW = air.aux.width();
  s.n_aux_instr = (uint32_t)prog_.aux_instr.size();
  const uint32_t AW = s.AW;
  // the periodic columns go up with the constants: every column's coefficients, then every column's table
  s.per_coef = (uint32_t)prog_.consts.size();
  std::vector<u64> tables;
  for (size_t c = 0; c < air.periodic.size(); c++) {
    const std::vector<u64> coef = air.periodic_coefficients(c), tab = p3_periodic_table(coef, k, lqd);
    prog_.consts.insert(prog_.consts.end(), coef.begin(), coef.end());
    tables.insert(tables.end(), tab.begin(), tab.end());
  }
  s.per_tab = (uint32_t)prog_.consts.size();
  prog_.consts.insert(prog_.consts.end(), tables.begin(), tables.end());
  s.per_val = (uint32_t)prog_.consts.size();
  if (AW)   // the term kernel reads the columns on the trace domain: their values, by row mod P
    for (const auto& pc : air.periodic) prog_.consts.insert(prog_.consts.end(), pc.values.begin(), pc.values.end());
  // FRI layers of at most 2^P3_TAIL_LOG values fold in one workgroup per proof
  s.tail_round = L > P3_TAIL_LOG ? std::min(k, L - P3_TAIL_LOG) : 0;
  for (int i = 0; i < 26; i++) {
    s.w[i] = gl::root_of_unity(i);
    s.w_inv[i] = gl::inv(s.w[i]);
  }
  const u64 w_q = gl::root_of_unity(k + lqd), gn = gl::pow(gl::GENERATOR, n);
  std::vector<u64> s_c(Q);
  for (size_t r = 0; r < Q; r++) {
    s.zh[r] = gl::sub(gl::mul(gn, gl::pow(w_q, r * n)), 1);
    s.zh_inv[r] = gl::inv(s.zh[r]);
    s_c[r] = gl::mul(gl::GENERATOR, gl::pow(w_q, r));
    s.s_inv[r] = gl::inv(s_c[r]);
  }
  s.g_inv = gl::inv(gl::root_of_unity(k));
  zfirst_inv_.assign(Q * Q, 0);
  for (size_t c = 0; c < Q; c++)
    for (size_t j = 0; j < Q; j++)
      if (j != c) zfirst_inv_[c * Q + j] = gl::inv(gl::sub(gl::pow(gl::mul(s_c[c], s.s_inv[j]), n), 1));
  s.o_aux = 8 + 4 * W + 4 * (uint32_t)Q + 4 * PW;
  s.o_fri = s.o_aux + (AW ? 4 + 8 * AW : 0);
  s.hdr_words = s.o_fri + 4 * k;
  s.o_points = s.hdr_words;
  s.o_apow = s.o_points + 2 * (2 + (uint32_t)Q);
  s.o_betas = s.o_apow + 2 * (2 * W + 2 * (uint32_t)Q + 2 * PW + 4 * AW);
  s.o_idx = s.o_betas + 2 * k;
  s.o_chal = s.o_idx + (num_queries + 1) / 2;
  s.hdr_stride = s.o_chal + 2 * s.NC;
  s.sz_a = 0;
  for (int r = 0; r < k; r++) s.sz_a += 2 + 4 * (L - r - 1);
  s.sz_b = W + 4 * L + 2 * (uint32_t)Q + 4 * L + (PW ? PW + 4 * L : 0) + (AW ? 2 * AW + 4 * L : 0);
  if ((size_t)s.hdr_words + (size_t)num_queries * (s.sz_a + s.sz_b) + 3 !=
      cfg_.num_inputs() + p3_preprocessed_words((int)PW, k, B, num_queries) +
          p3_aux_words((int)AW, k, B, num_queries))   // the public values follow
    throw std::logic_error("p3 device prover: flattened size mismatch");
  budget_bytes_ = P3_SCRATCH_BUDGET_BYTES;
}
P3ProverDev::~P3ProverDev() {
  if (impl_) {
    try {
      sync();
    } catch (...) {
    }
    delete impl_;
  }
}

// The carve-up of a group's scratch, written once: the buffers of G proofs from `base`, and the words they take.  A null
// base gives the size alone (no pointer is formed).  Every term is linear in G.
struct P3Carve {
  P3Bufs b;
  size_t words;
};
static P3Carve carve_scratch(const P3Shape& s, size_t G, u64* base) {
  const size_t n = (size_t)1 << s.k, N2 = (size_t)1 << s.L, W = s.W, Q2 = 2 * (size_t)s.Q, A2 = 2 * (size_t)s.AW;
  P3Carve c{};
  auto take = [&](size_t words) {
    u64* r = base ? base + c.words : nullptr;
    c.words += words;
    return r;
  };
  static_assert(sizeof(P3State) % 8 == 0, "P3State is an array of words");
  c.b.state = reinterpret_cast<P3State*>(take(G * (sizeof(P3State) / 8)));
  c.b.hdr = take(G * s.hdr_stride);
  c.b.tvals = take(G * W * n);
  c.b.tmp = take(G * std::max(std::max(W, Q2), A2) * n);   // also the terms the auxiliary scan works on
  c.b.tcoef = take(G * W * n);
  c.b.qv = take(G * Q2 * n);
  c.b.qcoef = take(G * Q2 * n);
  c.b.tlde = take(G * W * N2);
  c.b.qlde = take(G * Q2 * N2);
  c.b.ttree = take(G * 8 * N2);
  c.b.qtree = take(G * 8 * N2);
  c.b.layers = take(G * 4 * N2);
  c.b.ftrees = take(G * 8 * N2);
  if (A2) {   // the challenge phase of a handle with auxiliary columns; nothing for any other handle
    c.b.avals = take(G * A2 * n);
    c.b.acoef = take(G * A2 * n);
    c.b.alde = take(G * A2 * N2);
    c.b.atree = take(G * 8 * N2);
    c.b.atot = take(G * A2 * ((n + P3_AUX_SCAN_BLOCK - 1) / P3_AUX_SCAN_BLOCK));
  }
  return c;
}
size_t P3ProverDev::scratch_words_per_proof() const { return carve_scratch(shape_, 1, nullptr).words; }
size_t P3ProverDev::group_size(size_t n_proofs) const {
  size_t g = budget_bytes_ / (scratch_words_per_proof() * 8);
  g = std::max<size_t>(1, std::min<size_t>(g, 4096));
  return std::min(g, n_proofs);
}

size_t P3ProverDev::preprocessed_table_words() const {
  const size_t n = (size_t)1 << shape_.k, N2 = (size_t)1 << shape_.L;
  // a handle with auxiliary columns keeps the columns' values on the trace domain as well (PW n words, the last of the
  // tables): its term kernel reads them
  return shape_.PW ? shape_.PW * n + shape_.PW * N2 + 8 * N2 + (shape_.AW ? shape_.PW * n : 0) : 0;
}

// The preprocessed columns' tables, by the launches the trace takes with a group of one: rows -> columns -> coefficients ->
// LDE on 7 H_{n 2^B} in bit-reversed order -> tree.  The values and an NTT temporary (PW n words each) are freed behind a
// synchronisation; so is everything but the root when `keep` is false.  Blocks the host: it runs once per handle.
void P3ProverDev::ensure_preprocessed(bool keep, hipStream_t st) {
  if (!shape_.PW || impl_->prep.words || (!keep && prep_root_known_)) return;
  const P3Shape& s = shape_;
  const size_t n = (size_t)1 << s.k, N2 = (size_t)1 << s.L, PW = s.PW;
  DevMem tables(preprocessed_table_words()), rows(PW * n), vals_tmp(s.AW ? 0 : PW * n), tmp(PW * n);
  if (!impl_->prep_root.words) impl_->prep_root = DevMem(4);
  u64 *coef = tables.p, *lde = coef + PW * n, *tree = lde + PW * N2;
  u64* vals = s.AW ? tree + 8 * N2 : vals_tmp.p;   // kept behind the tree for the term kernel, or a temporary
  if (impl_->recorded) P25_HIP(hipStreamWaitEvent(st, impl_->done, 0));
  P25_HIP(hipMemcpyAsync(rows.p, prep_values_.data(), PW * n * 8, hipMemcpyHostToDevice, st));
  P3Shape ts = s;    // the transpose reads k, W and G alone
  ts.W = (uint32_t)PW;
  ts.G = 1;
  P3Bufs tb{};
  tb.tvals = vals;
  p3_launch_transpose(rows.p, PW * n, ts, tb, st);
  NttTables& nt = impl_->tables;
  ntt_inverse(nt, vals, n, false, tmp.p, n, coef, n, (int)s.k, (int)PW, 1, st);
  if (s.B <= 3) {
    ntt_lde_bitrev(nt, coef, n, lde, N2, (int)s.k, (int)s.B, (int)PW, gl::GENERATOR, st);
  } else {   // 16 cosets as two interleaved sets of 8, as run_group's lde
    ntt_lde_bitrev(nt, coef, n, lde, N2, (int)s.k, 3, (int)PW, gl::GENERATOR, st);
    ntt_lde_bitrev(nt, coef, n, lde + N2 / 2, N2, (int)s.k, 3, (int)PW, gl::mul(gl::GENERATOR, gl::root_of_unity(s.L)), st);
  }
  p3_launch_commit_cols(lde, PW * N2, 2 * N2, N2, (uint32_t)PW, N2, tree, 8 * N2, 1, st);
  P25_HIP(hipGetLastError());
  P25_HIP(hipMemcpyAsync(impl_->prep_root.p, tree + p3_level_off(N2, s.L), 32, hipMemcpyDeviceToDevice, st));
  P25_HIP(hipMemcpyAsync(prep_root_, tree + p3_level_off(N2, s.L), 32, hipMemcpyDeviceToHost, st));
  P25_HIP(hipStreamSynchronize(st));
  prep_root_known_ = true;
  if (keep) {
    impl_->prep = std::move(tables);
    // a handle without auxiliary columns keeps the host's copy until its checker's tables stand (ensure_check_tables)
    if (s.AW || impl_->check_tab.words) {
      prep_values_.clear();
      prep_values_.shrink_to_fit();
    }
  }
}
void P3ProverDev::preprocessed_commit(u64 out[4]) {
  if (!shape_.PW) throw std::invalid_argument("p25_p3_prover_preprocessed_commit: the prover's AIR has no preprocessed columns");
  ensure_impl();
  ensure_preprocessed(false, impl_->host_stream());
  for (int i = 0; i < 4; i++) out[i] = prep_root_[i];
}

double P3ProverDev::aux_stage_ms() {
  if (!shape_.AW || !impl_ || !impl_->aux_t1.e) throw std::invalid_argument("p25_p3_prover_aux_stage_ms: no proof with auxiliary columns has been made");
  P25_HIP(hipEventSynchronize(impl_->aux_t1));
  float ms = 0;
  P25_HIP(hipEventElapsedTime(&ms, impl_->aux_t0, impl_->aux_t1));
  return ms;
}

void P3ProverDev::sync() {
  if (!impl_ || !impl_->recorded) return;
  P25_HIP(hipEventSynchronize(impl_->done));
}

void P3ProverDev::ensure_impl() {
  if (!impl_) {
    std::unique_ptr<P3ProverImpl> im(new P3ProverImpl());
    im->prog = DevMem((prog_.instr.size() * sizeof(P3Instr) + 7) / 8);
    im->consts = DevMem(prog_.consts.size());
    if (!prog_.aux_instr.empty()) {
      im->aux_prog = DevMem((prog_.aux_instr.size() * sizeof(P3Instr) + 7) / 8);
      P25_HIP(hipMemcpy(im->aux_prog.p, prog_.aux_instr.data(), prog_.aux_instr.size() * sizeof(P3Instr), hipMemcpyHostToDevice));
    }
    im->zfirst = DevMem(zfirst_inv_.size());
    P25_HIP(hipMemcpy(im->prog.p, prog_.instr.data(), prog_.instr.size() * sizeof(P3Instr), hipMemcpyHostToDevice));
    P25_HIP(hipMemcpy(im->consts.p, prog_.consts.data(), prog_.consts.size() * 8, hipMemcpyHostToDevice));
    P25_HIP(hipMemcpy(im->zfirst.p, zfirst_inv_.data(), zfirst_inv_.size() * 8, hipMemcpyHostToDevice));
    im->done.create(hipEventDisableTiming);
    impl_ = im.release();
  }
}

void P3ProverDev::prove_dev(const u64* d_traces, size_t trace_stride, const u64* d_public, size_t n_proofs,
                            const u64* d_pow_starts, u64* d_inputs, size_t input_stride, uint32_t* d_status, hipStream_t st) {
  if (!n_proofs) return;
  ensure_impl();
  ensure_preprocessed(true, st);
  const size_t G = group_size(n_proofs), need = G * scratch_words_per_proof();
  if (impl_->scratch.words < need) {
    sync();   // an earlier call may still be using the old allocation
    impl_->scratch.regrow(need);
  }
  // the scratch is one region: wait, on the device, for the call before, whichever stream it went to; and leave the
  // record for the next call behind whatever this one managed to enqueue, also when it throws half way
  if (impl_->recorded) P25_HIP(hipStreamWaitEvent(st, impl_->done, 0));
  P3CallRecord record{impl_, st};
  for (size_t g0 = 0; g0 < n_proofs; g0 += G) {
    const size_t cnt = std::min(G, n_proofs - g0);
    // every per-proof array advances by the group's first proof: the kernels index inside the group
    run_group(d_traces + g0 * trace_stride, trace_stride, shape_.n_public ? d_public + g0 * shape_.n_public : nullptr,
              (uint32_t)cnt, d_pow_starts ? d_pow_starts + g0 : nullptr, d_inputs + g0 * input_stride, input_stride,
              d_status + g0, st);
  }
  P25_HIP(hipGetLastError());
}

P3Bufs P3ProverDev::group_bufs(const P3Shape& s, uint32_t G, const u64* d_public) const {
  const size_t n = (size_t)1 << s.k, N2 = (size_t)1 << s.L;
  const P3Carve carve = carve_scratch(s, G, impl_->scratch.p);
  if (carve.words != G * scratch_words_per_proof() || carve.words > impl_->scratch.words)
    throw std::logic_error("p3 device prover: a group's scratch is out of step with the per-proof figure");
  P3Bufs b = carve.b;
  b.prog = reinterpret_cast<const P3Instr*>(impl_->prog.p);
  b.consts = impl_->consts.p;
  b.zfirst_inv = impl_->zfirst.p;
  b.pub = d_public;
  if (s.PW && impl_->prep.words) {   // the handle's constant tables: the same pointers for every group
    b.pcoef = impl_->prep.p;
    b.plde = b.pcoef + (size_t)s.PW * n;
    b.ptree = b.plde + (size_t)s.PW * N2;
    if (s.AW) b.pvals = b.ptree + 8 * N2;
  }
  b.aux_prog = reinterpret_cast<const P3Instr*>(impl_->aux_prog.p);
  return b;
}

void P3ProverDev::run_group(const u64* d_traces, size_t trace_stride, const u64* d_public, uint32_t G, const u64* d_pow_starts,
                            u64* d_inputs, size_t input_stride, uint32_t* d_status, hipStream_t st) {
  P3Shape s = shape_;
  s.G = G;
  const int k = s.k, B = s.B;
  const size_t n = (size_t)1 << k, N2 = (size_t)1 << s.L, W = s.W, Q = s.Q, Q2 = 2 * Q;
  NttTables& tb = impl_->tables;
  const P3Bufs b = group_bufs(s, G, d_public);

  // the LDE on shift * <w_{n 2^B}> in bit-reversed order; 16 cosets as two interleaved sets of 8 (coset 2 c + e of the
  // first kind is coset c of the set with shift * w^e, and lands in half e of the bit-reversed output)
  auto lde = [&](const u64* coeffs, u64* out, int n_polys, u64 shift) {
    if (B <= 3) {
      ntt_lde_bitrev(tb, coeffs, n, out, N2, k, B, n_polys, shift, st);
    } else {
      ntt_lde_bitrev(tb, coeffs, n, out, N2, k, 3, n_polys, shift, st);
      ntt_lde_bitrev(tb, coeffs, n, out + N2 / 2, N2, k, 3, n_polys, gl::mul(shift, gl::root_of_unity(s.L)), st);
    }
  };

  // trace: columns -> coefficients (kept for the openings) -> LDE on 7 H_{n 2^B} -> tree   (p3_prover.cpp:208-218)
  p3_launch_transpose(d_traces, trace_stride, s, b, st);
  ntt_inverse(tb, b.tvals, n, false, b.tmp, n, b.tcoef, n, k, (int)(G * W), 1, st);
  lde(b.tcoef, b.tlde, (int)(G * W), gl::GENERATOR);
  p3_launch_commit_cols(b.tlde, W * N2, 2 * N2, N2, (uint32_t)W, N2, b.ttree, 8 * N2, G, st);
  p3_launch_chain(s, b, P3_CH_TRACE, 0, st);                       // observe the root, sample alpha -- or the challenges
  if (s.AW) {   // the challenge phase: terms, running sums, then the trace's commit on 2 AW columns per proof
    const int A2 = 2 * (int)s.AW;
    impl_->aux_t0.ensure();
    impl_->aux_t1.ensure();
    P25_HIP(hipEventRecord(impl_->aux_t0, st));
    p3_launch_aux_columns(s, b, st);
    ntt_inverse(tb, b.avals, n, false, b.tmp, n, b.acoef, n, k, (int)G * A2, 1, st);
    lde(b.acoef, b.alde, (int)G * A2, gl::GENERATOR);
    p3_launch_commit_cols(b.alde, (size_t)A2 * N2, 2 * N2, N2, (uint32_t)A2, N2, b.atree, 8 * N2, G, st);
    p3_launch_chain(s, b, P3_CH_AUX, 0, st);                       // observe the auxiliary root, sample alpha
    P25_HIP(hipEventRecord(impl_->aux_t1, st));
  }
  // quotient on 7 H_{n 2^lqd}, split into chunks; chunk c: iNTT on H_n, LDE with shift 7 / s_c   (:231-290)
  p3_launch_quotient(s, b, st);
  ntt_inverse(tb, b.qv, n, true, b.tmp, n, b.qcoef, n, k, (int)(G * Q2), 1, st);
  for (size_t c = 0; c < Q; c++)
    lde(b.qcoef + c * G * 2 * n, b.qlde + c * G * 2 * N2, (int)(2 * G), gl::mul(gl::GENERATOR, s.s_inv[c]));
  p3_launch_commit_cols(b.qlde, 2 * N2, (size_t)G * 2 * N2, N2, (uint32_t)Q2, N2, b.qtree, 8 * N2, G, st);
  p3_launch_chain(s, b, P3_CH_QUOTIENT, 0, st);                    // observe the root, sample zeta
  p3_launch_openings(s, b, st);                                    // :296-329
  p3_launch_chain(s, b, P3_CH_FRI_ALPHA, 0, st);
  p3_launch_reduced(s, b, st);                                     // :331-355
  for (uint32_t r = 0; r < s.tail_round; r++) {                    // :359-387
    p3_launch_commit_rows4(b.layers + p3_layer_off(N2, r), 4 * N2, N2 >> (r + 1), b.ftrees + p3_ftree_off(N2, r), 8 * N2, G, st);
    p3_launch_chain(s, b, P3_CH_FRI_ROUND, r, st);
    p3_launch_fold(s, b, r, st);
  }
  p3_launch_fri_tail(s, b, st);
  p3_launch_pow_search(s, b, d_pow_starts, st);                    // :394-400
  p3_launch_chain(s, b, P3_CH_QUERIES, 0, st);                     // :401-404
  p3_launch_gather(s, b, d_inputs, input_stride, d_status, st);    // :423-445
}

// ---------------------------------------------------------------------------------------------------------------------
// Checking a trace (include/p25.h "CHECKING A TRACE")
// ---------------------------------------------------------------------------------------------------------------------
size_t P3ProverDev::check_words() const { return p3ck_words(shape_.AW, n_constraints_); }

P3CheckArgs P3ProverDev::check_args() const {
  const P3Shape& s = shape_;
  P3CheckArgs a{};
  a.prog = prog_.instr.data();
  a.aux_prog = prog_.aux_instr.data();
  a.consts = prog_.consts.data();
  a.per_val = per_values_.data();
  a.n_instr = s.n_instr;
  a.n_aux_instr = s.n_aux_instr;
  a.n_constraints = n_constraints_;
  a.k = s.k; a.W = s.W; a.PW = s.PW; a.AW = s.AW; a.n_public = s.n_public;
  return a;
}

// The periodic and preprocessed values of a handle without auxiliary columns, on the device for its checker: made by its
// first check (one with such columns has them for its term kernel: P3Shape::per_val, P3Bufs::pvals).  Blocks the host.
void P3ProverDev::ensure_check_tables(hipStream_t st) {
  const P3Shape& s = shape_;
  const size_t n = (size_t)1 << s.k, per = per_values_.size(), words = per + (size_t)s.PW * n;
  if (s.AW || !words || impl_->check_tab.words) return;
  if (s.PW && prep_values_.size() != s.PW * n) throw std::logic_error("p3 device prover: the preprocessed values are gone");
  std::vector<u64> host(per_values_);
  host.resize(words);
  for (size_t r = 0; r < n; r++)
    for (size_t c = 0; c < s.PW; c++) host[per + c * n + r] = prep_values_[r * s.PW + c];
  DevMem tab(words);
  P25_HIP(hipMemcpyAsync(tab.p, host.data(), words * 8, hipMemcpyHostToDevice, st));
  P25_HIP(hipStreamSynchronize(st));
  impl_->check_tab = std::move(tab);
  if (impl_->prep.words) {   // the proving side has its tables: nothing reads the host's copy any more
    prep_values_.clear();
    prep_values_.shrink_to_fit();
  }
}

void P3ProverDev::check_dev(const u64* d_traces, size_t trace_stride, const u64* d_public, size_t n_proofs, u64* d_report,
                            size_t report_stride, hipStream_t st) {
  if (!n_proofs) return;
  ensure_impl();
  const P3Shape& sh = shape_;
  if (sh.AW) ensure_preprocessed(true, st);   // the transcript observes the preprocessed root; the terms read the values
  ensure_check_tables(st);
  const size_t G = group_size(n_proofs), need = G * scratch_words_per_proof();
  if (impl_->scratch.words < need) {
    sync();   // an earlier call may still be using the old allocation
    impl_->scratch.regrow(need);
  }
  if (impl_->recorded) P25_HIP(hipStreamWaitEvent(st, impl_->done, 0));   // one scratch, one ordering: as prove_dev
  P3CallRecord record{impl_, st};
  const int k = sh.k, B = sh.B;
  const size_t n = (size_t)1 << k, N2 = (size_t)1 << sh.L, W = sh.W;
  NttTables& tb = impl_->tables;
  P3CheckArgs a = check_args();
  a.prog = reinterpret_cast<const P3Instr*>(impl_->prog.p);
  a.aux_prog = reinterpret_cast<const P3Instr*>(impl_->aux_prog.p);
  a.consts = impl_->consts.p;
  for (size_t g0 = 0; g0 < n_proofs; g0 += G) {
    P3Shape s = sh;
    s.G = (uint32_t)std::min(G, n_proofs - g0);
    const P3Bufs b = group_bufs(s, s.G, sh.n_public ? d_public + g0 * sh.n_public : nullptr);
    p3_launch_transpose(d_traces + g0 * trace_stride, trace_stride, s, b, st);
    if (s.AW) {   // run_group's launches up to the scans: the challenges hang on the trace's commitment
      ntt_inverse(tb, b.tvals, n, false, b.tmp, n, b.tcoef, n, k, (int)(s.G * W), 1, st);
      if (B <= 3) {
        ntt_lde_bitrev(tb, b.tcoef, n, b.tlde, N2, k, B, (int)(s.G * W), gl::GENERATOR, st);
      } else {
        ntt_lde_bitrev(tb, b.tcoef, n, b.tlde, N2, k, 3, (int)(s.G * W), gl::GENERATOR, st);
        ntt_lde_bitrev(tb, b.tcoef, n, b.tlde + N2 / 2, N2, k, 3, (int)(s.G * W), gl::mul(gl::GENERATOR, gl::root_of_unity(s.L)), st);
      }
      p3_launch_commit_cols(b.tlde, W * N2, 2 * N2, N2, (uint32_t)W, N2, b.ttree, 8 * N2, s.G, st);
      p3_launch_chain(s, b, P3_CH_TRACE, 0, st);
      p3_launch_aux_columns(s, b, st);
    }
    P3CheckBatch bt{};
    bt.tvals = b.tvals;
    bt.avals = b.avals;
    bt.pub = b.pub;
    bt.chal = b.hdr + s.o_chal;
    bt.chal_stride = s.hdr_stride;
    bt.state = b.state;
    bt.report = d_report + g0 * report_stride;
    bt.report_stride = report_stride;
    a.per_val = s.AW ? impl_->consts.p + s.per_val : impl_->check_tab.p;
    a.pvals = s.AW ? b.pvals : impl_->check_tab.p + per_values_.size();
    p3_launch_check(a, bt, s.G, st);
  }
  P25_HIP(hipGetLastError());
}

void P3ProverDev::check_host(const u64* traces, const u64* public_values, size_t n_proofs, u64* report_out, size_t report_stride) {
  if (!n_proofs) return;
  const size_t tw = trace_words(), np = shape_.n_public, cw = check_words();
  ensure_impl();
  hipStream_t st = impl_->host_stream();
  DevMem d_traces(n_proofs * tw), d_pub(n_proofs * np), d_rep(n_proofs * cw);
  P25_HIP(hipMemcpyAsync(d_traces.p, traces, n_proofs * tw * 8, hipMemcpyHostToDevice, st));
  if (np) P25_HIP(hipMemcpyAsync(d_pub.p, public_values, n_proofs * np * 8, hipMemcpyHostToDevice, st));
  check_dev(d_traces.p, tw, np ? d_pub.p : nullptr, n_proofs, d_rep.p, cw, st);
  // the report_stride - check_words words behind a report stay untouched
  P25_HIP(hipMemcpy2DAsync(report_out, report_stride * 8, d_rep.p, cw * 8, cw * 8, n_proofs, hipMemcpyDeviceToHost, st));
  P25_HIP(hipStreamSynchronize(st));
}

void P3ProverDev::prove_host(const u64* traces, const u64* public_values, size_t n_proofs, const u64* pow_starts,
                             u64* inputs_out, size_t input_stride, int32_t* statuses) {
  if (!n_proofs) return;
  const size_t tw = trace_words(), ni = num_inputs(), np = shape_.n_public;
  ensure_impl();
  hipStream_t st = impl_->host_stream();
  DevMem d_traces(n_proofs * tw), d_pub(n_proofs * np), d_pow(n_proofs), d_out(n_proofs * ni), d_status((n_proofs + 1) / 2);
  P25_HIP(hipMemcpyAsync(d_traces.p, traces, n_proofs * tw * 8, hipMemcpyHostToDevice, st));
  if (np) P25_HIP(hipMemcpyAsync(d_pub.p, public_values, n_proofs * np * 8, hipMemcpyHostToDevice, st));
  if (pow_starts) P25_HIP(hipMemcpyAsync(d_pow.p, pow_starts, n_proofs * 8, hipMemcpyHostToDevice, st));
  prove_dev(d_traces.p, tw, np ? d_pub.p : nullptr, n_proofs, pow_starts ? d_pow.p : nullptr, d_out.p, ni, reinterpret_cast<uint32_t*>(d_status.p), st);
  // the input_stride - num_inputs words behind a proof stay untouched
  P25_HIP(hipMemcpy2DAsync(inputs_out, input_stride * 8, d_out.p, ni * 8, ni * 8, n_proofs, hipMemcpyDeviceToHost, st));
  statuses_to_host(reinterpret_cast<const uint32_t*>(d_status.p), n_proofs, statuses, st);
}

}  // namespace p25
