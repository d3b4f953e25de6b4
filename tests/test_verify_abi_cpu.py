"""CPU: the verifier's two entry points in the C ABI (include/p25.h: p25_verify_batch, p25_verify_batch_dev).

They are device entry points: the device is selected before the arguments are looked at, so a box without a GPU answers
P25_ERR_NO_DEVICE whatever it is given (there is no CPU path), and a GPU box refuses the same arguments before any launch.
Only arguments the library refuses on the host are passed, and never a device pointer: nothing here can reach a kernel."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT

OK, INVALID_ARG, NO_DEVICE = 0, 1, 2
REJECTS = {"P25_REJECT_VANISHING": 20, "P25_REJECT_POW": 21, "P25_REJECT_MALFORMED": 22, "P25_REJECT_INITIAL_MERKLE": 23,
           "P25_REJECT_FRI_EVAL": 24, "P25_REJECT_FRI_MERKLE": 25, "P25_REJECT_FINAL_POLY": 26}


def _gpu():
    import torch
    return torch.cuda.is_available()


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


def _header_enum():
    text = open(os.path.join(ROOT, "include", "p25.h")).read()
    return {name: int(value) for name, value in re.findall(r"\b(P25_(?:OK|ERR|WARN|REJECT)_?\w*)\s*=\s*(\d+)", text)}


def test_symbols_are_exported_and_bound(p25):
    lib = p25.lib()
    for name in ("p25_verify_batch", "p25_verify_batch_dev"):
        assert name in p25.EXPORTED_SYMBOLS
        fn = getattr(lib, name)
        assert fn.restype is C.c_int32 and len(fn.argtypes) == 7
    assert callable(p25.Circuit.verify) and callable(p25.Circuit.verify_dev)


def test_status_values_are_distinct_and_match_the_header(p25):
    enum = _header_enum()
    for name, value in REJECTS.items():
        assert enum[name] == value
        assert getattr(p25.binding, name[len("P25_"):]) == value
        assert p25.binding.STATUS_NAMES[value] == name[len("P25_"):]
    assert len(set(enum.values())) == len(enum), "two status names share a value"
    # the oracle's verifier codes 10, 11, 13..16 plus ten; 22 is the library's own
    assert sorted(REJECTS.values()) == list(range(20, 27))


@pytest.fixture(scope="module")
def fx(p25):
    c = p25.Circuit.build_gadget(0, 0)
    pw = int(c.info.proof_words)
    return p25.lib(), c, pw, np.zeros(pw, dtype=np.uint64), np.zeros(1, dtype=np.int32), np.zeros(4, dtype=np.uint64), \
        np.zeros(64, dtype=np.uint64)


CASES = {
    # name -> (reason on a GPU box, call(lib, h, pw, proof, status, digest, cap))
    "host/circuit": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch(None, None, None, _p(pr), 1, pw, _p(st))),
    "host/proofs": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch(h, None, None, None, 1, pw, _p(st))),
    "host/status": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch(h, None, None, _p(pr), 1, pw, None)),
    "host/digest_alone": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch(h, _p(dg), None, _p(pr), 1, pw, _p(st))),
    "host/cap_alone": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch(h, None, _p(cap), _p(pr), 1, pw, _p(st))),
    "host/stride": ("proof_stride smaller", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch(h, None, None, _p(pr), 1, pw - 1, _p(st))),
    "dev/circuit": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch_dev(None, None, None, None, 1, pw, None)),
    "dev/proofs": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch_dev(h, None, None, None, 1, pw, None)),
    "dev/digest_alone": ("null argument", lambda l, h, pw, pr, st, dg, cap: l.p25_verify_batch_dev(h, _p(dg), None, None, 0, pw, None)),
}


@pytest.mark.parametrize("case", sorted(CASES))
def test_verify_entry_points_check_the_device_first(fx, case):
    lib, c, pw, proof, status, digest, cap = fx
    text, call = CASES[case]
    st = call(lib, c._h, pw, proof, status, digest, cap)
    if not _gpu():
        assert st == NO_DEVICE
        assert "no CPU fallback" in lib.p25_last_error().decode()
    else:
        assert st == INVALID_ARG
        assert text in lib.p25_last_error().decode()
    assert (status == 0).all() and (proof == 0).all()
