"""CPU: the argument rules of p25_p3_verify_batch[_dev] (include/p25.h).  Argument errors need no device and come first;
an empty batch touches nothing; everything else answers P25_ERR_NO_DEVICE here: the library has no CPU verifier."""
import ctypes as C

import numpy as np
import pytest

import p3_verify_cases as pc

OK, INVALID_ARG, NO_DEVICE = 0, 1, 2


def _gpu():
    import torch
    return torch.cuda.is_available()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _last(p25):
    return p25.lib().p25_last_error().decode()


@pytest.fixture(scope="module")
def fx(p25):
    case = pc.flip_case(p25, pc.FIB334)
    pr = case.prover(p25)
    yield pr, np.array(case.words), np.full(1, 77, dtype=np.int32)
    pr.close()


def test_status_codes_in_the_header(p25):
    import os
    import re
    from conftest import ROOT
    hdr = open(os.path.join(ROOT, "include", "p25.h")).read()
    want = {"MALFORMED": 30, "POW": 31, "INPUT_MERKLE": 32, "FRI_MERKLE": 33, "FINAL_POLY": 34, "CONSTRAINTS": 35}
    for name, value in want.items():
        assert re.search(r"P25_P3_REJECT_%s\s*=\s*%d\b" % (name, value), hdr), name


def test_null_arguments_are_refused(p25, fx):
    lib = p25.lib()
    pr, words, st = fx
    ni = pr.num_inputs
    cases = {
        "null handle": lambda: lib.p25_p3_verify_batch(None, _p(words), 1, ni, _p(st)),
        "null inputs": lambda: lib.p25_p3_verify_batch(pr._h, None, 1, ni, _p(st)),
        "null statuses": lambda: lib.p25_p3_verify_batch(pr._h, _p(words), 1, ni, None),
        "dev null handle": lambda: lib.p25_p3_verify_batch_dev(None, _p(words), 1, ni, _p(st), None),
        "dev null inputs": lambda: lib.p25_p3_verify_batch_dev(pr._h, None, 1, ni, _p(st), None),
        "dev null statuses": lambda: lib.p25_p3_verify_batch_dev(pr._h, _p(words), 1, ni, None, None),
        "scratch query null handle": lambda: lib.p25_p3_prover_scratch_bytes(None, None, None),
    }
    for name, call in cases.items():
        assert call() == INVALID_ARG, name
        assert "null" in _last(p25), name
    assert st[0] == 77


def test_short_stride_is_refused(p25, fx):
    lib = p25.lib()
    pr, words, st = fx
    ni = pr.num_inputs
    assert lib.p25_p3_verify_batch(pr._h, _p(words), 1, ni - 1, _p(st)) == INVALID_ARG and "input_stride" in _last(p25)
    assert lib.p25_p3_verify_batch_dev(pr._h, _p(words), 1, ni - 1, _p(st), None) == INVALID_ARG and "input_stride" in _last(p25)
    assert lib.p25_p3_verify_batch(pr._h, _p(words), 1, 0, _p(st)) == INVALID_ARG
    assert st[0] == 77


def test_empty_batch_touches_nothing(p25):
    lib = p25.lib()
    pr = pc.flip_case(p25, pc.FIB334).prover(p25)       # a fresh handle: nothing has allocated on it
    assert lib.p25_p3_verify_batch(pr._h, None, 0, 0, None) == OK
    assert lib.p25_p3_verify_batch_dev(pr._h, None, 0, 0, None, None) == OK
    assert lib.p25_p3_verify_batch(None, None, 0, 0, None) == INVALID_ARG     # the handle is checked first, as for proving
    assert pr.scratch_bytes() == (0, 0)
    pr.close()


def test_compute_needs_a_device(p25, fx):
    lib = p25.lib()
    pr, words, st = fx
    s = lib.p25_p3_verify_batch(pr._h, _p(words), 1, pr.num_inputs, _p(st))
    if _gpu():
        assert s == OK and st[0] == OK
        st[0] = 77
    else:
        assert s == NO_DEVICE and "no CPU fallback" in _last(p25)
        assert lib.p25_p3_verify_batch_dev(pr._h, _p(words), 1, pr.num_inputs, _p(st), None) == NO_DEVICE
        assert st[0] == 77 and pr.scratch_bytes() == (0, 0)
        with pytest.raises(p25.P25Error) as e:
            pr.verify(words)
        assert e.value.status == NO_DEVICE
