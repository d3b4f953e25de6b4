#!/usr/bin/env python3
"""Device plonky3 prover against the host prover, per proof, on the same box.

Fibonacci AIR, 100 queries, 16 proof-of-work bits, log_n in {12, 16, 20} (--log-n to choose), batches of 1 and 16 with
distinct pow_starts.  For each shape:
  * device: P3Prover.prove_dev on device-resident traces, one warm-up call (tables, scratch, code objects), then the timed
    calls; the time is a host clock around enqueue + P3Prover.sync(), i.e. it ends in a device synchronise;
  * host: p3_prove_fibonacci(threads=16), the unchanged yardstick, once per distinct pow_start that is compared;
  * the device rows are asserted equal to the host's, word for word.
Writes one JSON (default profiles/p3_prover_bench.json) and prints it as one line; exits non-zero if the device form is not
faster per proof than the host form at the largest log_n of the run.  There is no CPU path: without a GPU the
first compute call raises.

--prep-machine LOG_N adds the cost of preprocessed columns (include/p25.h, PREPROCESSED COLUMNS) at one shape: a width-1
machine next0 = local0 + sel c with sel, c two preprocessed columns, against the same width and degree without columns
(next0 = local0^2 + 3); 2^LOG_N rows, the largest batch of --batches.  Reported under "preprocessed": the one-off build of
the handle's tables (first p25_p3_prover_preprocessed_commit on a fresh handle, after another handle has loaded the code
objects; it includes that handle's own constant tables) and the device time per proof with and without columns; the rows
with columns are asserted equal to the host prover's.

--aux-lookup LOG_N adds the cost of challenge-phase auxiliary columns (include/p25.h, AUXILIARY COLUMNS) at one shape: the
LogUp range check of a trace column f into the preprocessed table 0..n-1 with a multiplicity column m (one challenge, one
auxiliary column) beside the plain constraint c = f m, against the same AIR with the auxiliary parts removed (c = f m
alone); 2^LOG_N rows, the largest batch of --batches.  Reported under "aux" and written to profiles/p3_aux.json as well: ms
per proof for both, and the share of the call that the term + scan + auxiliary-commit stage takes (HIP events around it,
P3Prover.aux_stage_ms); the last row with auxiliary columns is asserted equal to the host prover's.

--check measures the trace checker (include/p25.h, CHECKING A TRACE) INSTEAD of the shapes above: P3Prover.check_dev beside
P3Prover.prove_dev on the same device-resident batch of 16 satisfying traces, for two AIRs -- `whens` (width 2, two public
values, one constraint of each `when` kind) at 2^12 rows, and the --aux-lookup LogUp range check (one auxiliary column) at
2^--check-lookup-log-n rows.  HIP events around each call on one stream, one warm-up, the median of 5; every report is
asserted to say "no violation" and every proof to succeed.  Written to profiles/p3_check.json (--check-out).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

P = 0xFFFFFFFF00000001


def fib_trace(log_n):
    n = 1 << log_n
    t = np.zeros((n, 3), dtype=np.uint64)
    a, b = 1, 1
    for i in range(n):
        c = a + b
        if c >= P:
            c -= P
        t[i] = (a, b, c)
        a, b = b, c
    return t


def machine(p25, log_n, with_columns):
    """-> (air, trace[n][1], public values[2]) of the --prep-machine shape."""
    n = 1 << log_n
    rng = np.random.default_rng(4242)
    prep = rng.integers(0, P, size=(n, 2), dtype=np.uint64)
    prep[:, 0] &= np.uint64(1)
    air = p25.Air(1, n_public=2, preprocessed=prep if with_columns else None)
    x = air.local(0)
    air.when_first_row(air.sub(x, air.public(0)))
    step = air.add(x, air.mul(air.prep_local(0), air.prep_local(1))) if with_columns else air.add(air.mul(x, x), air.const(3))
    air.when_transition(air.sub(air.next(0), step))
    air.when_last_row(air.sub(x, air.public(1)))
    t = np.zeros((n, 1), dtype=np.uint64)
    v = 5
    for i in range(n):
        t[i, 0] = v
        v = (v + int(prep[i, 0]) * int(prep[i, 1])) % P if with_columns else (v * v + 3) % P
    return air, t, np.array([int(t[0, 0]), int(t[n - 1, 0])], dtype=np.uint64)


def bench_preprocessed(p25, torch, dev, args):
    log_n, b = args.prep_machine, max(args.batches)
    out = {"log_n": log_n, "batch": b, "columns": 2}
    for with_columns in (True, False):
        air, trace, pv = machine(p25, log_n, with_columns)
        pr = p25.P3Prover(air, log_n, 1, args.queries, args.pow_bits)
        ni = pr.num_inputs
        d_traces = torch.from_numpy(trace.view(np.int64).copy()).to(dev).reshape(1, -1).repeat(b, 1).contiguous()
        d_pv = torch.from_numpy(pv.view(np.int64).copy()).to(dev).reshape(1, -1).repeat(b, 1).contiguous()
        d_inputs = torch.zeros((b, ni), dtype=torch.int64, device=dev)
        d_status = torch.zeros(b, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call():
            pr.prove_dev(d_traces.data_ptr(), trace.size, b, 0, d_inputs.data_ptr(), ni, d_status.data_ptr(),
                         d_public_values=d_pv.data_ptr())
            pr.sync()

        call()   # warm-up: code objects, scratch, the handle's tables
        if with_columns:
            fresh = p25.P3Prover(air, log_n, 1, args.queries, args.pow_bits)
            t0 = time.perf_counter()
            root = fresh.preprocessed_commit()
            out["table_build_s"] = time.perf_counter() - t0
            assert root.tolist() == pr.preprocessed_commit().tolist()
            fresh.close()
        times = []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
        assert d_status.cpu().numpy().tolist() == [0] * b, "device prover reported a failure"
        if with_columns:
            row, _cfg = p25.p3_prove_air(air, trace, num_queries=args.queries, pow_bits=args.pow_bits, threads=args.threads,
                                         public_values=pv)
            assert np.array_equal(d_inputs.cpu().numpy().view(np.uint64)[b - 1], row), "proof differs from the host prover's"
        key = "with_columns" if with_columns else "without_columns"
        out[key] = {"num_inputs": ni, "gpu_call_s": [round(t, 6) for t in times], "gpu_s_per_proof": float(np.median(times)) / b}
        pr.close()
    return out


def lookup(p25, log_n, with_aux):
    """-> (air, trace[n][3]) of the --aux-lookup shape."""
    n = 1 << log_n
    f = np.random.default_rng(777).integers(0, n, n, dtype=np.uint64)
    m = np.bincount(f.astype(np.int64), minlength=n).astype(np.uint64)
    trace = np.ascontiguousarray(np.stack([f, m, f * m % np.uint64(P)], axis=1))   # f m < 2^28: no wrap before the reduction
    table = np.arange(n, dtype=np.uint64).reshape(-1, 1)
    air = p25.Air(3, preprocessed=table, aux=1 if with_aux else 0)
    lf, lm, t = air.local(0), air.local(1), air.prep_local(0)
    air.assert_zero(air.sub(air.local(2), air.mul(lf, lm)))
    if with_aux:
        g = air.challenge(0)
        gf, gt = air.sub(g, lf), air.sub(g, t)
        num, den = air.sub(air.mul(lm, gf), gt), air.mul(gt, gf)
        j = air.aux_column(num, den)
        air.when_first_row(air.aux_local(j))
        air.assert_zero(air.sub(air.mul(air.sub(air.aux_next(j), air.aux_local(j)), den), num))
    else:
        air.when_first_row(air.sub(t, t))   # keeps the preprocessed column read, as the auxiliary form reads it
    return air, trace


def bench_aux(p25, torch, dev, args):
    log_n, b = args.aux_lookup, max(args.batches)
    out = {"log_n": log_n, "batch": b, "queries": args.queries, "pow_bits": args.pow_bits, "device": torch.cuda.get_device_name(0)}
    for with_aux in (True, False):
        air, trace = lookup(p25, log_n, with_aux)
        pr = p25.P3Prover(air, log_n, 1, args.queries, args.pow_bits)
        ni = pr.num_inputs
        d_traces = torch.from_numpy(trace.view(np.int64).copy()).to(dev).reshape(1, -1).repeat(b, 1).contiguous()
        d_inputs = torch.zeros((b, ni), dtype=torch.int64, device=dev)
        d_status = torch.zeros(b, dtype=torch.int32, device=dev)
        torch.cuda.synchronize()

        def call():
            pr.prove_dev(d_traces.data_ptr(), trace.size, b, 0, d_inputs.data_ptr(), ni, d_status.data_ptr())
            pr.sync()

        call()   # warm-up: code objects, scratch, the handle's tables
        times, stage = [], []
        for _ in range(args.reps):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            call()
            times.append(time.perf_counter() - t0)
            if with_aux:
                stage.append(pr.aux_stage_ms() / 1e3)
        assert d_status.cpu().numpy().tolist() == [0] * b, "device prover reported a failure"
        key = "with_aux" if with_aux else "without_aux"
        out[key] = {"num_inputs": ni, "gpu_call_s": [round(t, 6) for t in times], "gpu_ms_per_proof": 1e3 * float(np.median(times)) / b}
        if with_aux:
            row, _cfg = p25.p3_prove_air(air, trace, num_queries=args.queries, pow_bits=args.pow_bits, threads=args.threads)
            assert np.array_equal(d_inputs.cpu().numpy().view(np.uint64)[b - 1], row), "proof differs from the host prover's"
            out[key]["aux_stage_s"] = [round(t, 6) for t in stage]
            out[key]["aux_stage_share"] = float(np.median(stage)) / float(np.median(times))
        pr.close()
    return out


def whens(p25, log_n):
    """-> (air, trace[n][2], public values[2]): b (b - 1) always, x = PUBLIC(0) on the first row, x' = x + b on transitions,
    x = PUBLIC(1) on the last row; random bits in b."""
    n = 1 << log_n
    air = p25.Air(2, n_public=2)
    x, b = air.local(0), air.local(1)
    air.assert_zero(air.mul(b, air.sub(b, air.const(1))))
    air.when_first_row(air.sub(x, air.public(0)))
    air.when_transition(air.sub(air.sub(air.next(0), x), b))
    air.when_last_row(air.sub(x, air.public(1)))
    bits = np.random.default_rng(31).integers(0, 2, n, dtype=np.uint64)
    xs = np.uint64(1000) + np.concatenate([np.zeros(1, dtype=np.uint64), np.cumsum(bits[:-1], dtype=np.uint64)])
    return air, np.ascontiguousarray(np.stack([xs, bits], axis=1)), np.array([1000, int(xs[-1])], dtype=np.uint64)


def bench_check(p25, torch, dev, args):
    b, reps = 16, 5
    out = {"tool": "tools/p3_prover_bench.py --check", "batch": b, "queries": args.queries, "pow_bits": args.pow_bits,
           "timing": "HIP events around one call on one stream; one warm-up call of each, then the median of %d" % reps,
           "device": torch.cuda.get_device_name(0), "airs": {}}
    shapes = [("whens", 12, whens(p25, 12)), ("logup_range", args.check_lookup_log_n, lookup(p25, args.check_lookup_log_n, True) + (None,))]
    for name, log_n, (air, trace, pv) in shapes:
        pr = p25.P3Prover(air, log_n, 1, args.queries, args.pow_bits)
        ni, cw = pr.num_inputs, pr.check_words
        d_traces = torch.from_numpy(trace.view(np.int64).copy()).to(dev).reshape(1, -1).repeat(b, 1).contiguous()
        d_pv = None if pv is None else torch.from_numpy(pv.view(np.int64).copy()).to(dev).reshape(1, -1).repeat(b, 1).contiguous()
        pvp = 0 if d_pv is None else d_pv.data_ptr()
        d_inputs = torch.zeros((b, ni), dtype=torch.int64, device=dev)
        d_status = torch.zeros(b, dtype=torch.int32, device=dev)
        d_report = torch.zeros((b, cw), dtype=torch.int64, device=dev)
        stream = torch.cuda.Stream()
        sp = stream.cuda_stream

        def prove():
            pr.prove_dev(d_traces.data_ptr(), trace.size, b, 0, d_inputs.data_ptr(), ni, d_status.data_ptr(), stream=sp,
                         d_public_values=pvp)

        def check():
            pr.check_dev(d_traces.data_ptr(), trace.size, b, d_report.data_ptr(), cw, stream=sp, d_public_values=pvp)

        def timed(call):
            call()   # warm-up: code objects, scratch, the handle's tables
            stream.synchronize()
            ms = []
            for _ in range(reps):
                t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                t0.record(stream)
                call()
                t1.record(stream)
                t1.synchronize()
                ms.append(t0.elapsed_time(t1))
            return ms

        torch.cuda.synchronize()
        prove_ms, check_ms = timed(prove), timed(check)
        assert d_status.cpu().numpy().tolist() == [0] * b, "device prover reported a failure"
        rep_words = d_report.cpu().numpy().view(np.uint64)
        assert (rep_words[:, 0] == 0).all() and (rep_words[:, 1] == 0).all(), "the checker reports a violation in a satisfying trace"
        out["airs"][name] = {"log_n": log_n, "width": int(air.width), "constraints": len(air.constraints),
                             "aux_columns": len(air.aux_columns), "num_inputs": ni, "check_words": cw,
                             "prove_call_ms": [round(t, 4) for t in prove_ms], "check_call_ms": [round(t, 4) for t in check_ms],
                             "prove_ms_per_proof": float(np.median(prove_ms)) / b, "check_ms_per_proof": float(np.median(check_ms)) / b}
        pr.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, nargs="+", default=[12, 16, 20])
    ap.add_argument("--batches", type=int, nargs="+", default=[1, 16])
    ap.add_argument("--queries", type=int, default=100)
    ap.add_argument("--pow-bits", type=int, default=16)
    ap.add_argument("--reps", type=int, default=3, help="timed device calls per shape (the median is reported)")
    ap.add_argument("--host-proofs", type=int, default=2, help="distinct host proofs timed and compared per log_n")
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--prep-machine", type=int, default=0, metavar="LOG_N",
                    help="also measure an AIR with two preprocessed columns at 2^LOG_N rows (0 = off)")
    ap.add_argument("--aux-lookup", type=int, default=0, metavar="LOG_N",
                    help="also measure the LogUp range check with one auxiliary column at 2^LOG_N rows (0 = off)")
    ap.add_argument("--aux-out", default=os.path.join(ROOT, "profiles", "p3_aux.json"))
    ap.add_argument("--check", action="store_true",
                    help="measure check_dev beside prove_dev (whens at 2^12, the LogUp range check) and nothing else")
    ap.add_argument("--check-lookup-log-n", type=int, default=14)
    ap.add_argument("--check-out", default=os.path.join(ROOT, "profiles", "p3_check.json"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "p3_prover_bench.json"))
    args = ap.parse_args()

    import torch
    p25 = entry.load_package()
    p25.device_init(0)
    dev = torch.device("cuda", 0)
    if args.check:
        result = bench_check(p25, torch, dev, args)
        os.makedirs(os.path.dirname(os.path.abspath(args.check_out)), exist_ok=True)
        with open(args.check_out, "w") as f:
            json.dump(result, f, indent=1)
            f.write("\n")
        print(json.dumps(result))
        return
    air = p25.Air.fibonacci()
    result = {"tool": "tools/p3_prover_bench.py", "air": "fibonacci", "queries": args.queries, "pow_bits": args.pow_bits,
              "host_threads": args.threads, "device": torch.cuda.get_device_name(0), "shapes": []}
    for log_n in args.log_n:
        trace = fib_trace(log_n)
        pr = p25.P3Prover(air, log_n, 1, args.queries, args.pow_bits)
        ni = pr.num_inputs
        max_b = max(args.batches)
        starts = np.array([(i * 0x9E3779B97F4A7C15) % (P - (1 << 40)) for i in range(max_b)], dtype=np.uint64)
        starts[0] = 0
        # host yardstick: time and keep the first few distinct proofs
        host_rows, host_s = {}, []
        for i in range(min(args.host_proofs, max_b)):
            t0 = time.perf_counter()
            row, _cfg = p25.p3_prove_fibonacci(log_n, args.queries, args.pow_bits, pow_start=int(starts[i]), threads=args.threads)
            host_s.append(time.perf_counter() - t0)
            host_rows[i] = row
        host_per_proof = float(np.median(host_s))
        d_trace = torch.from_numpy(trace.view(np.int64).copy()).to(dev)
        for b in args.batches:
            # the batch proves the SAME trace b times from b pow_starts: distinct proofs, one device copy of the trace each
            d_traces = d_trace.reshape(1, -1).repeat(b, 1).contiguous()
            d_starts = torch.from_numpy(starts[:b].view(np.int64).copy()).to(dev)
            d_inputs = torch.zeros((b, ni), dtype=torch.int64, device=dev)
            d_status = torch.zeros(b, dtype=torch.int32, device=dev)
            torch.cuda.synchronize()

            def call():
                pr.prove_dev(d_traces.data_ptr(), trace.size, b, d_starts.data_ptr(), d_inputs.data_ptr(), ni,
                             d_status.data_ptr())
                pr.sync()

            call()   # warm-up
            times = []
            for _ in range(args.reps):
                d_inputs.zero_()
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                call()
                times.append(time.perf_counter() - t0)
            got = d_inputs.cpu().numpy().view(np.uint64)
            assert d_status.cpu().numpy().tolist() == [0] * b, "device prover reported a failure"
            for i, row in host_rows.items():
                if i < b:
                    assert np.array_equal(got[i], row), f"log_n {log_n}, batch {b}: proof {i} differs from the host prover's"
            per_proof = float(np.median(times)) / b
            result["shapes"].append({"log_n": log_n, "batch": b, "num_inputs": ni, "gpu_call_s": [round(t, 6) for t in times],
                                     "gpu_s_per_proof": per_proof, "host_s_per_proof": host_per_proof,
                                     "host_s": [round(t, 6) for t in host_s], "host_over_gpu": host_per_proof / per_proof,
                                     "rows_compared_equal": min(len(host_rows), b)})
            del d_traces, d_inputs
        pr.close()
    if args.prep_machine:
        result["preprocessed"] = bench_preprocessed(p25, torch, dev, args)
    if args.aux_lookup:
        result["aux"] = bench_aux(p25, torch, dev, args)
        os.makedirs(os.path.dirname(args.aux_out), exist_ok=True)
        with open(args.aux_out, "w") as f:
            json.dump(dict(result["aux"], tool="tools/p3_prover_bench.py --aux-lookup"), f, indent=1)
            f.write("\n")
    # the acceptance for speed: per proof, the device form beats the host form of the same run at the largest size
    top = max(args.log_n)
    result["acceptance"] = {"log_n": top, "gpu_faster_than_host": all(sh["host_over_gpu"] > 1.0 for sh in result["shapes"]
                                                                      if sh["log_n"] == top)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))
    if not result["acceptance"]["gpu_faster_than_host"]:
        sys.exit(f"the device prover is not faster per proof than the host prover at log_n {top}")


if __name__ == "__main__":
    main()
