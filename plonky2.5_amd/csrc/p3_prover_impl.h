// Internal: the device state of a p25_p3_prover handle, shared by its proving side (p3_prover_dev.hip) and its verifying
// side (p3_verify_dev.hip).
#pragma once
#include "p3_kernels.h"
#include "prover.h"

namespace p25 {

struct P3ProverImpl {
  NttTables tables;
  DevMem prog, consts, zfirst, scratch;
  DevEvent aux_t0, aux_t1;   // timing events around the challenge phase of the last group proved (P3ProverDev::aux_stage_ms)
  DevMem aux_prog;   // the auxiliary columns' terms' program (P3AirDevice::aux_instr); empty without such columns
  DevMem prep;       // the preprocessed columns' tables: coefficients | LDE | tree (p3_prover_dev.hip); empty until a proving call
  DevMem prep_root;  // the 4 words of the preprocessed commitment: all the verifying side keeps of the columns
  // the checker's value tables of a handle WITHOUT auxiliary columns: periodic values | preprocessed values [PW][n];
  // empty until its first check (a handle with such columns reads the term kernel's tables)
  DevMem check_tab;
  DevMem vscratch;   // the verifier's: challenge blocks and folded values (p3_verify_dev.hip)
  DevStream own_stream;   // the host entry points' (prove_host, verify_host): created by the first of them
  // Recorded behind the last launch of every compute call.  The next call's stream waits for it before it touches the
  // scratch, so calls on different streams take the one scratch region in turn; each call's record sits behind its wait
  // for the call before, so the latest record covers everything the prover has enqueued.
  DevEvent done;
  bool recorded = false;
  hipStream_t host_stream() {
    if (!own_stream) own_stream = DevStream(hipStreamNonBlocking);
    return own_stream;
  }
};

// Leaves the record for the next call behind whatever a compute call managed to enqueue, also when it throws half way.
struct P3CallRecord {
  P3ProverImpl* im;
  hipStream_t st;
  ~P3CallRecord() {
    if (hipEventRecord(im->done, st) == hipSuccess) im->recorded = true;
  }
};

}  // namespace p25
