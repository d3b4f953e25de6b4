"""Time p25_p3_verify_batch_dev against the two provers around it, in one process.

Two device-resident batches of inner plonky3 proofs, made by p25_p3_prove_batch_dev and left where it wrote them: 256
fib-64 proofs (the artifact's shape: 100 queries, 16 PoW bits) and 16 proofs of a 2^16-row Fibonacci trace (same
parameters).  Per batch: 5 warm-up and 20 timed verify_dev calls, each between two HIP events on the stream the call is
enqueued on, and the proving of the same batch by p25_p3_prove_batch_dev measured the same way.  For the fib-64 batch also
the outer p25_prove_batch_dev over the same proofs -- the step a screen would spare.  No threshold: the record states the
three times side by side.  One JSON object goes to --out (profiles/p3_verify_batch.json is the committed record) and to
stdout.

    python tools/p3_verify_bench.py [--warmup 5] [--steps 20] [--out profiles/p3_verify_batch.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch  # noqa: E402

import __graft_entry__ as ge  # noqa: E402

P = 0xFFFFFFFF00000001


def fib_trace(log_n):
    t = np.zeros((1 << log_n, 3), dtype=np.uint64)
    a, b = 1, 1
    for i in range(1 << log_n):
        c = (a + b) % P
        t[i] = (a, b, c)
        a, b = b, c
    return t


def event_ms(stream, enqueue):
    """Device milliseconds of what enqueue() puts on `stream`."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record(stream)
    enqueue()
    e1.record(stream)
    e1.synchronize()
    return e0.elapsed_time(e1)


def circuit_ms(circuit, side, enqueue):
    """The same for work a circuit spreads over its own streams (tools/verify_bench.py)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    circuit.stream_join(side.cuda_stream)
    e0.record(side)
    circuit.wait_stream(side.cuda_stream)
    enqueue()
    circuit.stream_join(side.cuda_stream)
    e1.record(side)
    e1.synchronize()
    return e0.elapsed_time(e1)


class Batch:
    """n device-resident proofs of the Fibonacci AIR with 2^log_n rows, proved on the device with distinct PoW starts."""

    def __init__(self, p25, dev, side, log_n, n):
        self.n, self.side = n, side
        self.pr = p25.P3Prover(p25.Air.fibonacci(), log_n, 1, 100, 16)
        self.ni = self.pr.num_inputs
        trace = fib_trace(log_n)
        self.tw = trace.size
        self.d_traces = torch.from_numpy(np.tile(trace.reshape(-1), n).view(np.int64)).to(dev)
        self.d_pow = torch.from_numpy(np.arange(n, dtype=np.int64) << 24).to(dev)
        self.d_inputs = torch.zeros(n * self.ni, dtype=torch.int64, device=dev)
        self.d_pst = torch.full((n,), -1, dtype=torch.int32, device=dev)
        self.d_vst = torch.full((n,), -1, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

    def prove(self):
        self.pr.prove_dev(self.d_traces.data_ptr(), self.tw, self.n, self.d_pow.data_ptr(), self.d_inputs.data_ptr(), self.ni,
                          self.d_pst.data_ptr(), self.side.cuda_stream)

    def verify(self):
        self.pr.verify_dev(self.d_inputs.data_ptr(), self.n, self.ni, self.d_vst.data_ptr(), self.side.cuda_stream)

    def measure(self, warmup, steps, prove_steps):
        prove_ms = [event_ms(self.side, self.prove) for _ in range(1 + prove_steps)][1:]    # the first allocates the scratch
        self.pr.sync()
        assert self.d_pst.cpu().tolist() == [0] * self.n
        for _ in range(warmup):
            event_ms(self.side, self.verify)
        verify_ms = [event_ms(self.side, self.verify) for _ in range(steps)]
        self.pr.sync()
        assert self.d_vst.cpu().tolist() == [0] * self.n, "the verifier rejects a proof of the batch"
        v, p = statistics.median(verify_ms), statistics.median(prove_ms)
        return {"proofs": self.n, "words_per_proof": self.ni, "verify_batch_ms_median": round(v, 3),
                "verify_batch_ms_min": round(min(verify_ms), 3), "verify_batch_ms_max": round(max(verify_ms), 3),
                "verify_us_per_proof": round(1000 * v / self.n, 2), "p3_prove_batch_ms_median": round(p, 2),
                "verify_share_of_p3_proving_percent": round(100 * v / p, 3),
                "verify_scratch_bytes": self.pr.scratch_bytes()[1]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--prove-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p3_verify_batch.json"))
    args = ap.parse_args()

    p25 = ge.load_package()
    p25.device_init(0)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream()
    small = Batch(p25, dev, side, 6, 256)
    fib64 = small.measure(args.warmup, args.steps, args.prove_steps)
    large = Batch(p25, dev, side, 16, 16)
    rows64k = large.measure(args.warmup, args.steps, args.prove_steps)

    # the outer prover over the fib-64 batch: what a rejected inner proof costs without the screen
    c = p25.Circuit.build_p3_verifier(p25.P3Config.fib64())
    pw = int(c.info.proof_words)
    d_seeds = torch.arange(small.n, dtype=torch.int64, device=dev)
    d_proofs = torch.zeros((small.n, pw), dtype=torch.int64, device=dev)
    d_status = torch.full((small.n,), -1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()

    def outer():
        c.prove_dev(small.d_inputs.data_ptr(), small.n, d_seeds.data_ptr(), d_proofs.data_ptr(), pw, d_status.data_ptr())

    outer_ms = [circuit_ms(c, side, outer) for _ in range(1 + args.prove_steps)][1:]
    c.sync()
    assert d_status.cpu().tolist() == [0] * small.n
    outer_med = statistics.median(outer_ms)
    fib64["outer_prove_batch_ms_median"] = round(outer_med, 1)
    fib64["verify_share_of_outer_proving_percent"] = round(100 * fib64["verify_batch_ms_median"] / outer_med, 4)

    result = {"tool": "tools/p3_verify_bench.py", "device": torch.cuda.get_device_name(0), "air": "Fibonacci, width 3",
              "num_queries": 100, "pow_bits": 16, "log_blowup": 1, "warmup": args.warmup, "steps": args.steps,
              "prove_steps": args.prove_steps, "fib64_x256": fib64, "rows_2_16_x16": rows64k}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
