"""Time p25_verify_batch_dev against proving the same batch, in one process.

256 fib-64 proofs are proved on the device and stay there; then 5 warm-up and 20 timed verify_dev calls over the batch,
each bracketed by HIP events on a side stream that is joined to the circuit's streams on both sides (stream_join /
wait_stream: no host synchronisation inside the bracket).  The proving time of the same batch is measured the same way
and is the comparison.  Also the latency of verifying a single proof.  One JSON object goes to --out
(profiles/verify_batch.json is the committed record) and to stdout.

    python tools/verify_bench.py [--batch 256] [--warmup 5] [--steps 20] [--out profiles/verify_batch.json]
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


def bracketed_ms(circuit, side, enqueue):
    """Device milliseconds of what enqueue() puts on the circuit's streams."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    circuit.stream_join(side.cuda_stream)
    e0.record(side)
    circuit.wait_stream(side.cuda_stream)
    enqueue()
    circuit.stream_join(side.cuda_stream)
    e1.record(side)
    e1.synchronize()
    return e0.elapsed_time(e1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--prove-steps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "verify_batch.json"))
    args = ap.parse_args()

    p25 = ge.load_package()
    p25.device_init(0)
    inputs, _ = p25.p3_proof_from_json(open(os.path.join(ROOT, "tests", "golden", "proof_fibonacci.json")).read())
    c = p25.Circuit.build_p3_verifier(p25.P3Config.fib64())
    c.digest()
    B, pw = args.batch, int(c.info.proof_words)
    dev = torch.device("cuda", 0)
    d_in = torch.from_numpy(np.stack([inputs] * B).view(np.int64)).to(dev)
    d_seeds = torch.arange(B, dtype=torch.int64, device=dev)
    d_proofs = torch.zeros((B, pw), dtype=torch.int64, device=dev)
    d_prove_status = torch.zeros(B, dtype=torch.int32, device=dev)
    d_status = torch.full((B,), -1, dtype=torch.int32, device=dev)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()

    def prove():
        c.prove_dev(d_in.data_ptr(), B, d_seeds.data_ptr(), d_proofs.data_ptr(), pw, d_prove_status.data_ptr())

    def verify(n):
        return lambda: c.verify_dev(d_proofs.data_ptr(), n, pw, d_status.data_ptr())

    prove_ms = [bracketed_ms(c, side, prove) for _ in range(1 + args.prove_steps)][1:]   # the first allocates the contexts
    c.sync()
    assert d_prove_status.cpu().tolist() == [0] * B
    for _ in range(args.warmup):
        bracketed_ms(c, side, verify(B))
    batch_ms = [bracketed_ms(c, side, verify(B)) for _ in range(args.steps)]
    c.sync()
    assert d_status.cpu().tolist() == [0] * B, "the verifier rejects a proof of the batch"
    for _ in range(args.warmup):
        bracketed_ms(c, side, verify(1))
    single_ms = [bracketed_ms(c, side, verify(1)) for _ in range(args.steps)]
    c.sync()

    prove_med, batch_med, single_med = (statistics.median(v) for v in (prove_ms, batch_ms, single_ms))
    result = {
        "tool": "tools/verify_bench.py", "device": torch.cuda.get_device_name(0), "circuit": "fib-64 plonky3 verifier",
        "batch": B, "proof_words": pw, "warmup": args.warmup, "steps": args.steps,
        "verify_batch_ms_median": round(batch_med, 3), "verify_batch_ms_min": round(min(batch_ms), 3),
        "verify_batch_ms_max": round(max(batch_ms), 3), "verify_us_per_proof": round(1000 * batch_med / B, 2),
        "prove_batch_ms_median": round(prove_med, 1), "prove_steps": args.prove_steps,
        "verify_share_of_proving_percent": round(100 * batch_med / prove_med, 3),
        "verify_single_proof_ms_median": round(single_med, 3),
    }
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(json.dumps(result, indent=1) + "\n")
    print(line)


if __name__ == "__main__":
    main()
