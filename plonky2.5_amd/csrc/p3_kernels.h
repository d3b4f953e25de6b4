// Internal: the device form of the plonky3 prover (p3_prover.cpp stage by stage) -- shapes, per-proof state and the
// launchers of kernels_p3.hip.  Every launcher takes the proofs of one GROUP as a grid dimension: one launch per stage for
// the whole group (p3_prover_dev.hip).
#pragma once
#include "kernels.h"
#include "p3_circuit.h"

namespace p25 {

// ---- the AIR as a register program (compiled by P3AirDevice::compile from the AirProgram DAG) ----
// Operands: kind << 28 | index.  LOCAL / NEXT / CONST / PUBLIC nodes never take a slot: they are re-read where they are
// used (PUBLIC: from the proof's own row of public values).  PERIODIC is as free: its index is log_period << 24 | the
// words of the columns before it (at most 31 * 256), and its value comes from the caller of run_air -- a table word in the
// quotient kernel, q_c(zeta^(n/P)) in the identity lanes.  PREP_LOCAL / PREP_NEXT (index = preprocessed column) are read
// through run_air's `load` like LOCAL / NEXT: from the handle's shared LDE in the quotient kernel, from the proof's
// preprocessed openings in the identity lanes.  CHALLENGE (index = challenge) is read from the proof's challenge words;
// AUX_LOCAL / AUX_NEXT (index = auxiliary column) through `load` again, which recomposes the column's two components.
// The three take no slot and stand only in programs that run in ExtF.
enum : uint32_t { P3_OPND_SLOT = 0, P3_OPND_LOCAL = 1, P3_OPND_NEXT = 2, P3_OPND_CONST = 3, P3_OPND_PUBLIC = 4,
                  P3_OPND_PERIODIC = 5, P3_OPND_PREP_LOCAL = 6, P3_OPND_PREP_NEXT = 7, P3_OPND_CHALLENGE = 8,
                  P3_OPND_AUX_LOCAL = 9, P3_OPND_AUX_NEXT = 10 };
// what run_air's load(which, column) is asked for: bit 0 the next row, bit 1 the preprocessed matrix, bit 2 the auxiliary one
enum : int { P3_LOAD_LOCAL = 0, P3_LOAD_NEXT = 1, P3_LOAD_PREP_LOCAL = 2, P3_LOAD_PREP_NEXT = 3, P3_LOAD_AUX_LOCAL = 4,
             P3_LOAD_AUX_NEXT = 5 };
GL_HD uint32_t p3_per_log_period(uint32_t index) { return index >> 24; }
GL_HD uint32_t p3_per_offset(uint32_t index) { return index & 0xffffffu; }
enum : uint32_t { P3_OP_ADD = 3, P3_OP_SUB = 4, P3_OP_MUL = 5, P3_OP_EMIT = 6 };  // ADD..MUL as AirProgram::Op
struct P3Instr {
  uint32_t op, dst /* slot; EMIT: the constraint's `when` */, a, b;
};
// The limits of the device form, refused by p25_p3_prover_create: the values of arithmetic nodes that are alive at the same
// time (after the host's liveness pass) live in a per-lane array of this many words.
constexpr uint32_t P3_MAX_LIVE = 64;
constexpr uint32_t P3_MAX_INSTR = 1u << 20;
// The launch forms of a Merkle tree (build_tree, kernels_p3.hip): a level with more than P3_TREE_COOP_MAX nodes over the
// whole group runs one lane per node, a smaller one 16 lanes per node; once a proof's level has at most P3_TREE_TOP_NODES
// nodes, one workgroup per proof finishes the tree.  FRI layers of at most 2^P3_TAIL_LOG values fold in one workgroup per
// proof (k_p3_fri_tail).  The tests read these three from this file and derive their shapes from them.
constexpr int P3_TREE_COOP_MAX = 1 << 16;
constexpr int P3_TREE_TOP_NODES = 16;
constexpr int P3_TAIL_LOG = 10;
// The prefix sum over an auxiliary column (k_p3_aux_scan_block / _totals / _finish, kernels_p3.hip): rows per block of the
// block-local scan, and block totals per tile of the totals pass, which walks its tiles one after the other in ONE
// workgroup per (proof, column).  The tests read these two from this file: the totals take a second tile from
// P3_AUX_SCAN_BLOCK * P3_AUX_TOTALS_TILE rows on.
constexpr int P3_AUX_SCAN_BLOCK = 256;
constexpr int P3_AUX_TOTALS_TILE = 256;

struct P3AirDevice {
  std::vector<P3Instr> instr;
  // for an AIR with auxiliary columns, their terms' program: it emits num_0, den_0, num_1, den_1, ... in column order and
  // shares `consts` (and the slots' limit) with the AIR's own
  std::vector<P3Instr> aux_instr;
  // the CONST nodes' values; P3ProverDev appends the periodic columns' coefficients and tables (P3Shape::per_coef, per_tab)
  std::vector<u64> consts;
  uint32_t max_live = 0;
  // throws std::invalid_argument naming the limit the program exceeds
  static P3AirDevice compile(const AirProgram& air);
};

// ---- per-proof device state ----
struct P3State {
  u64 st[12], inb[12], outb[12];  // the duplex challenger (src/p3/challenger.rs:70-169)
  uint32_t n_in, n_out;
  u64 alpha[2], zeta[2], fri_alpha[2], final_poly[2];
  u64 pow_witness;
  uint32_t status, pad;
};

// Shape of one proof and the layout of a group's scratch.  All offsets in words.
struct P3Shape {
  uint32_t k, B, L, lqd, Q, W, num_queries, pow_bits;
  uint32_t n_instr, tail_round;   // FRI rounds >= tail_round run in k_p3_fri_tail
  uint32_t G;                     // proofs of this group
  uint32_t n_public;              // public values per proof: the tail of its flat words
  // The periodic columns, behind the AIR's constants in P3Bufs::consts and shared by every proof of every group.  Column c
  // with `off` words of columns before it: its P coefficients at per_coef + off, its table of P Q values on the quotient
  // coset (p3_periodic_table) at per_tab + off * Q.
  uint32_t per_coef, per_tab;
  // The preprocessed columns: PW of them (0: none), in P3Bufs::pcoef / plde / ptree, shared like the periodic tables.
  uint32_t PW;
  // The challenge phase: NC challenges, AW auxiliary columns (0: none; then the chain runs the phases it ran), the
  // instructions of their terms' program, and per_val -- the periodic columns' VALUES on the trace domain, behind the
  // tables in P3Bufs::consts (column c at per_val + off, read by row mod P), which only the term kernel reads.
  uint32_t NC, AW, n_aux_instr, per_val;
  u64 w[26], w_inv[26];           // primitive 2^i-th roots of unity and their inverses
  u64 zh[8], zh_inv[8];           // x^n - 1 on the quotient coset, by chunk
  u64 s_inv[8];                   // 1 / s_c
  u64 g_inv;                      // 1 / w_n
  // hdr: the proof's first words (trace root | quotient root | trace_local | trace_next | chunks | prep_local | prep_next |
  // from o_aux: aux root | aux_local | aux_next | FRI roots from o_fri), then points (zeta, zeta w_n, zeta / s_c), powers of
  // fri_alpha, betas, query indices, the challenges from o_chal
  uint32_t hdr_words, o_fri, o_points, o_apow, o_betas, o_idx, hdr_stride, o_aux, o_chal;
  uint32_t sz_a, sz_b;            // words per query: commit-phase openings, input openings
};
struct P3Bufs {
  P3State* state;
  u64* hdr;
  u64 *tvals, *tmp, *tcoef, *tlde, *ttree;   // [G][W][n] x3, [G][W][N2], [G][8 N2]
  u64 *qv, *qcoef, *qlde, *qtree;            // [Q][G][2][n] x2, [Q][G][2][N2], [G][8 N2]
  u64 *layers, *ftrees;                      // [G][4 N2], [G][8 N2]
  const P3Instr* prog;
  const u64* consts;
  const u64* zfirst_inv;                     // [Q][Q]: 1 / Z_{D_j}(s_c)
  // [G][n_public]: the public values of THIS GROUP's proofs -- the batch's array advanced by the group's first proof, like
  // every other per-proof pointer of a group (blockIdx.y counts inside the group); null when n_public = 0
  const u64* pub;
  // The preprocessed columns' coefficients [PW][n], LDE on 7 H_{N2} in bit-reversed order [PW][N2] and tree (8 N2 words):
  // constant tables of the handle, made once on the device (P3ProverDev::ensure_preprocessed), the same for every proof
  // of every group -- no blockIdx.y offset ever applies to them; null when PW = 0
  const u64 *pcoef, *plde, *ptree;
  // The challenge phase, per proof of the group like the trace's buffers: the auxiliary matrix's 2 AW base columns on the
  // trace domain [G][2 AW][n] (column j's components at 2 j and 2 j + 1), coefficients, LDE on 7 H_{N2} in bit-reversed
  // order [G][2 AW][N2], tree [G][8 N2], and the scan's block totals [G][AW][2][blocks]; null when AW = 0
  u64 *avals, *acoef, *alde, *atree, *atot;
  const P3Instr* aux_prog;
  // the preprocessed columns' values on the trace domain [PW][n], kept by handles with auxiliary columns for the term kernel
  const u64* pvals;
};

// words of level l of a tree over h leaves (levels concatenated, 4 words per digest), FRI layer r, FRI tree r
GL_HD size_t p3_level_off(size_t h, unsigned l) { return 8 * (h - (h >> l)); }
GL_HD size_t p3_layer_off(size_t N2, unsigned r) { return 4 * (N2 - (N2 >> r)); }
GL_HD size_t p3_ftree_off(size_t N2, unsigned r) { return 8 * (N2 - (N2 >> r)); }

// P3_CH_AUX stands between TRACE and QUOTIENT for a handle with auxiliary columns: TRACE then ends with the challenges
// instead of alpha, and AUX observes the auxiliary root and samples alpha.
enum : uint32_t { P3_CH_TRACE = 0, P3_CH_QUOTIENT = 1, P3_CH_FRI_ALPHA = 2, P3_CH_FRI_ROUND = 3, P3_CH_QUERIES = 4, P3_CH_AUX = 5 };

void p3_launch_transpose(const u64* d_traces, size_t trace_stride, const P3Shape& s, const P3Bufs& b, hipStream_t st);
// leaves of the column matrix at base + g * proof_stride + (c >> 1) * pair_stride + (c & 1) * col_stride, then the tree
void p3_launch_commit_cols(const u64* base, size_t proof_stride, size_t pair_stride, size_t col_stride, uint32_t width,
                           size_t h, u64* tree, size_t tree_stride, uint32_t G, hipStream_t st);
// leaves = rows of 4 words, then the tree
void p3_launch_commit_rows4(const u64* rows, size_t rows_stride, size_t h, u64* tree, size_t tree_stride, uint32_t G,
                            hipStream_t st);
void p3_launch_chain(const P3Shape& s, const P3Bufs& b, uint32_t phase, uint32_t round, hipStream_t st);
// the auxiliary columns on the trace domain: terms (one inversion per row), then the exclusive prefix sum in three launches
void p3_launch_aux_columns(const P3Shape& s, const P3Bufs& b, hipStream_t st);
void p3_launch_quotient(const P3Shape& s, const P3Bufs& b, hipStream_t st);
void p3_launch_openings(const P3Shape& s, const P3Bufs& b, hipStream_t st);   // evaluations, then the identity check
void p3_launch_reduced(const P3Shape& s, const P3Bufs& b, hipStream_t st);
void p3_launch_fold(const P3Shape& s, const P3Bufs& b, uint32_t round, hipStream_t st);
void p3_launch_fri_tail(const P3Shape& s, const P3Bufs& b, hipStream_t st);
void p3_launch_pow_search(const P3Shape& s, const P3Bufs& b, const u64* d_pow_starts, hipStream_t st);
void p3_launch_gather(const P3Shape& s, const P3Bufs& b, u64* d_out, size_t out_stride, uint32_t* d_status, hipStream_t st);

// ---- the prover handle's device side (p3_prover_dev.hip) ----
// Default scratch budget of a prover: a batch runs in groups of as many proofs as fit (at least one).
constexpr size_t P3_SCRATCH_BUDGET_BYTES = (size_t)12 << 30;
// The verifier's buffer never grows past this: a larger batch is checked in chunks.
constexpr size_t P3_VERIFY_SCRATCH_BYTES = (size_t)32 << 20;
struct P3ProverImpl;
struct P3VerifyArgs;   // p3_verify_lanes.h
struct P3CheckArgs;    // p3_check_lanes.h
class P3ProverDev {
 public:
  // host only: validates as p3_prove_air does and compiles the AIR; throws std::invalid_argument
  P3ProverDev(const AirProgram& air, int log_n, int log_blowup, int num_queries, int pow_bits);
  ~P3ProverDev();
  const P3Config& config() const { return cfg_; }
  // words of a flat proof: the proof's in `add_virtual_to` order, then its n_public public values
  // (cfg_.num_inputs() + n_public without preprocessed columns; with them, their openings and third batches as well)
  size_t num_inputs() const {
    return (size_t)shape_.hdr_words + (size_t)shape_.num_queries * (shape_.sz_a + shape_.sz_b) + 3 + shape_.n_public;
  }
  uint32_t n_public() const { return shape_.n_public; }
  size_t trace_words() const { return ((size_t)1 << cfg_.log_trace_height) * (size_t)cfg_.trace_width; }
  size_t scratch_words_per_proof() const;
  size_t group_size(size_t n_proofs) const;
  // The preprocessed columns' constant tables (coefficients PW n, LDE PW N2, tree 8 N2 words): outside the group budget,
  // counted by scratch_bytes under `proving` once a proving call has made them.
  size_t preprocessed_table_words() const;
  uint32_t preprocessed_width() const { return shape_.PW; }
  // The 4 words of the preprocessed commitment as the device computed them (the first call computes them: a handle that
  // has only verified, or done nothing yet, makes the tables in a temporary and frees it).  Throws without columns.
  void preprocessed_commit(u64 out[4]);
  // The device time (HIP events) of the challenge phase -- terms, prefix sum, the auxiliary commit, its chain launch -- of
  // the LAST group the handle proved; waits for it.  Throws for a handle without auxiliary columns or before its first proof.
  double aux_stage_ms();
  void set_scratch_budget(size_t bytes) { budget_bytes_ = bytes ? bytes : P3_SCRATCH_BUDGET_BYTES; }
  // enqueue-only on `st`.  d_public: [n_proofs][n_public], packed (unread when n_public = 0)
  void prove_dev(const u64* d_traces, size_t trace_stride, const u64* d_public, size_t n_proofs, const u64* d_pow_starts,
                 u64* d_inputs, size_t input_stride, uint32_t* d_status, hipStream_t st);
  // host buffers (checked by the caller): copies, proves on the handle's own stream, waits
  void prove_host(const u64* traces, const u64* public_values, size_t n_proofs, const u64* pow_starts, u64* inputs_out,
                  size_t input_stride, int32_t* statuses);
  void sync();
  // The verifying side (p3_verify_dev.hip, kernels_p3_verify.hip): src/p3/verifier.rs on flat proofs of this handle's AIR and
  // shape.  Takes none of the proving scratch; its own buffer holds verify_scratch_words_per_proof() words per proof of a
  // chunk, and a chunk is what fits min(the scratch budget, P3_VERIFY_SCRATCH_BYTES) -- at least one proof.
  size_t verify_scratch_words_per_proof() const;
  size_t verify_chunk(size_t n_proofs) const;
  // enqueue-only on `st`; d_status[i] = 0 or a P25_P3_REJECT_* code
  void verify_dev(const u64* d_inputs, size_t n_proofs, size_t input_stride, uint32_t* d_status, hipStream_t st);
  // host buffers (checked by the caller): copies, verifies on the handle's own stream, waits
  void verify_host(const u64* inputs, size_t n_proofs, size_t input_stride, int32_t* statuses);
  // the batch description without the batch (host pointers to the AIR program): also what the host driver of the lane
  // functions starts from (tests/native/p3_verify_lanes.cpp)
  P3VerifyArgs verify_args() const;
  // bytes of device scratch the handle holds now, by side
  void scratch_bytes(size_t* proving, size_t* verifying) const;
  // The checking side (kernels_p3_check.hip, p3_check_lanes.h; include/p25.h "CHECKING A TRACE"): which constraint a trace
  // breaks and where, without a proof.  Runs in the proving scratch, group by group like a proving call: the transpose,
  // and for a handle with auxiliary columns the proving call's own launches up to the scans, then the check.  The first
  // check of a handle WITHOUT auxiliary columns puts the periodic and preprocessed values on the device (such a handle
  // keeps them nowhere else); scratch_bytes counts them under `proving` from then on.
  size_t check_words() const;
  // enqueue-only on `st`; report i = check_words() words at d_report + i * report_stride
  void check_dev(const u64* d_traces, size_t trace_stride, const u64* d_public, size_t n_proofs, u64* d_report,
                 size_t report_stride, hipStream_t st);
  // host buffers (checked by the caller): copies, checks on the handle's own stream, waits
  void check_host(const u64* traces, const u64* public_values, size_t n_proofs, u64* report_out, size_t report_stride);
  // the check as far as the handle decides it (host pointers to the programs and the tables): what the host checker
  // (p3_check.cpp) and the host driver of the lane functions (tests/native/p3_check_lanes.cpp) start from
  P3CheckArgs check_args() const;

 private:
  void ensure_impl();
  // the preprocessed tables on the device, made on `st` behind the handle's earlier work: keep = false computes the root
  // in a temporary (the verifying side needs nothing else); no-op once done or without columns
  void ensure_preprocessed(bool keep, hipStream_t st);
  // the buffers of a group of G proofs in the handle's scratch, and the handle's constant tables
  P3Bufs group_bufs(const P3Shape& s, uint32_t G, const u64* d_public) const;
  void ensure_check_tables(hipStream_t st);
  void run_group(const u64* d_traces, size_t trace_stride, const u64* d_public, uint32_t G, const u64* d_pow_starts,
                 u64* d_inputs, size_t input_stride, uint32_t* d_status, hipStream_t st);
  P3Config cfg_;
  P3AirDevice prog_;
  P3Shape shape_;
  std::vector<u64> zfirst_inv_;
  std::vector<u64> prep_values_;   // [n][PW] row-major, until the device has them
  std::vector<u64> per_values_;    // the periodic columns' values, column after column: what a check reads by row mod P
  uint32_t n_constraints_ = 0;
  u64 prep_root_[4] = {0, 0, 0, 0};
  bool prep_root_known_ = false;
  size_t budget_bytes_;
  P3ProverImpl* impl_ = nullptr;   // device state, made by the first compute call
};

}  // namespace p25
