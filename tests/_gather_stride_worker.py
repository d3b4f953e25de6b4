"""Worker for tests/test_gpu_device_entry_points.py: p25_gather_proofs in a world of one, at a stride above the proof.

The library's own communicator (p25_comm_init: librccl on its own side stream), one process, one GPU; started as a child
of the test like tests/_nccl_worker.py.  p25_gather_proofs moves whole strides: all n * proof_stride_words words of the
source arrive, padding included, and nothing lands outside the destination."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as ge  # noqa: E402
from device_buffers import Banded, Banded32  # noqa: E402
from oracle_binding import splitmix_field  # noqa: E402


def main():
    p25 = ge.load_package()
    p25.device_init(0)
    c = p25.Circuit.build_gadget(0, 0)
    pw, n = int(c.info.proof_words), 5
    stride = pw + 5
    # real proofs at that stride, written by p25_prove_batch_dev: the gather is ordered behind them by a mark
    xs, ys = splitmix_field(n, seed=61), splitmix_field(n, seed=62)
    inp = np.stack([xs, ys, xs & ys], axis=1)
    inp[3, 2] += np.uint64(1)                                   # one proof fails: its status travels too
    d_in, d_seeds = Banded(3 * n), Banded(n)
    d_in.set(inp)
    d_seeds.set(np.arange(n, dtype=np.uint64))
    d_proofs, d_status = Banded(n * stride, before=4097), Banded32(n, before=4097)
    d_all, d_all_status = Banded(n * stride, before=4097), Banded32(n)
    comm = p25.Comm(p25.comm_unique_id(), 0, 1)
    c.prove_dev(d_in.ptr, n, d_seeds.ptr, d_proofs.ptr, stride, d_status.ptr)
    c.mark(0)
    comm.gather(c, 0, d_proofs.ptr, stride, d_status.ptr, [n], 0, d_all.ptr, d_all_status.ptr)
    comm.sync()
    c.sync()
    torch.cuda.synchronize()
    src, dst = d_proofs.get(), d_all.get()
    assert d_status.get().tolist() == [0, 0, 0, 4, 0], d_status.get().tolist()
    assert (dst == src).all(), "the gathered block differs from the source"          # padding (sentinels) included
    pad = (np.arange(n)[:, None] * stride + np.arange(pw, stride)[None, :]).ravel()
    d_proofs.assert_untouched(pad)
    assert (dst[pad] == src[pad]).all() and (dst[pad] >= np.uint64(0xFFFFFFFF00000001)).all()
    ref, st = c.prove(inp, seeds=np.arange(n, dtype=np.uint64))
    assert st.tolist() == [0, 0, 0, 4, 0]
    got = dst.reshape(n, stride)[:, :pw]
    for i in (0, 1, 2, 4):
        assert (got[i] == ref[i]).all(), i
    assert (d_all_status.get() == d_status.get()).all()
    for b in (d_proofs, d_status, d_all, d_all_status):
        b.assert_bands_intact()
    d_in.assert_unchanged()
    d_seeds.assert_unchanged()
    comm.close()
    c.close()
    print("GATHER_STRIDE_OK", torch.cuda.get_device_name(0))


if __name__ == "__main__":
    main()
