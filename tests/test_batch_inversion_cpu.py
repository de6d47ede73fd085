"""Batch inversion (FiniteField::batch_inversion, math/traits.rs:93-121) and inverse_or_zero (:39-45): the parts that need no GPU --
the exported symbols, the argument errors every flavour returns before any HIP call, the C++ mirror's self-test program, and the
expected-value builder the GPU tests compare against (tests/inversion_ref.py), pinned here against tests/pyref and the oracle."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests import inversion_ref, pyref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twenty-first_amd", "host")

NEW = ("tf_batch_inversion_bfe", "tf_batch_inversion_xfe", "tf_batch_inversion_bfe_dev", "tf_batch_inversion_xfe_dev",
       "tf_batch_inversion_bfe_dev_async", "tf_batch_inversion_xfe_dev_async", "tf_inverse_or_zero_bfe", "tf_inverse_or_zero_xfe",
       "tf_inverse_or_zero_bfe_dev", "tf_inverse_or_zero_xfe_dev")
OK, NULL = 0, 7


def _p(a):
    return C.c_void_p(a.ctypes.data)


def test_symbols_declared_and_exported(tf):
    from twenty_first_amd import _lib

    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    lib = tf.lib()
    for name in NEW:
        assert name + "(" in header, name
        assert name in _lib.SIGNATURES, name
        assert hasattr(lib, name), name
    assert lib.tf_version() == 1002  # new entry points are found by their symbols, not by a version bump


@pytest.mark.parametrize("suffix", ["bfe", "xfe"])
def test_host_argument_errors_without_device(tf, suffix):
    lib = tf.lib()
    w = 1 if suffix == "bfe" else 3
    x = np.ones(4 * w, dtype=np.uint64)
    out = np.zeros(4 * w, dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    host = getattr(lib, f"tf_batch_inversion_{suffix}")
    dev = getattr(lib, f"tf_batch_inversion_{suffix}_dev")
    dev_async = getattr(lib, f"tf_batch_inversion_{suffix}_dev_async")
    oz_host = getattr(lib, f"tf_inverse_or_zero_{suffix}")
    oz_dev = getattr(lib, f"tf_inverse_or_zero_{suffix}_dev")
    # a NULL pointer with n > 0
    for fn in (host, oz_host):
        assert fn(None, 4, _p(out)) == NULL
        assert fn(_p(x), 4, None) == NULL
    for fn in (dev, oz_dev):
        assert fn(None, 4, _p(out), None) == NULL
        assert fn(_p(x), 4, None, None) == NULL
    assert dev_async(None, 4, _p(out), None, _p(st)) == NULL
    assert dev_async(_p(x), 4, None, None, _p(st)) == NULL
    assert dev_async(_p(x), 4, _p(out), None, None) == NULL
    # n == 0: TF_OK, nothing touched (NULL pointers included)
    for fn in (host, oz_host):
        assert fn(None, 0, None) == OK
        assert fn(_p(x), 0, _p(out)) == OK
    for fn in (dev, oz_dev):
        assert fn(None, 0, None, None) == OK
    assert dev_async(None, 0, None, None, None) == OK
    assert not out.any() and st[0] == 0


def test_python_shapes_are_checked_on_the_host(tf):
    with pytest.raises(ValueError):
        tf.batch_inversion(np.ones(4, dtype=np.uint64), width=3)
    with pytest.raises(ValueError):
        tf.inverse_or_zero(np.ones(3, dtype=np.uint64), width=2)
    assert tf.batch_inversion(np.zeros(0, dtype=np.uint64)).size == 0  # n == 0 never reaches a device
    assert tf.inverse_or_zero(np.zeros(0, dtype=np.uint64), width=3).size == 0


def test_expected_value_builder_agrees_with_pyref_and_the_oracle(oracle):
    rng = np.random.default_rng(7)
    # base field: the raw-word formula against pyref's modular inverse and the oracle's BFieldElement::inverse
    xs = [int(v) for v in oracle.fill_random(300, 0x1A7)] + [oracle.bfe_new(v) for v in (1, 2, 3, 100, inversion_ref.P - 1)]
    for raw in xs:
        want = inversion_ref.bfe_inv_raw(raw)
        assert want == oracle.bfe_inverse(raw)
        assert want == pyref.to_raw(pow(pyref.to_val(raw), inversion_ref.P - 2, inversion_ref.P))
    # extension field: random elements, lifted base-field elements (a, 0, 0), (0, a, 0), (0, 0, a) and x itself
    w = oracle.fill_random(3 * 200, 0x1A8)
    elems = [w[3 * i:3 * i + 3] for i in range(200)]
    for a in oracle.fill_random(20, 0x1A9):
        for k in range(3):
            e = np.zeros(3, dtype=np.uint64)
            e[k] = a
            elems.append(e)
    elems.append(np.array([0, oracle.bfe_new(1), 0], dtype=np.uint64))
    for e in elems:
        want = np.array(inversion_ref.xfe_inv_raw(e.tolist()), dtype=np.uint64)
        assert np.array_equal(want, oracle.xfe_inverse(e))
    for e in elems[::4]:  # Fermat over p^3 is slow in Python: every fourth element
        vals = tuple(pyref.to_val(int(r)) for r in e)
        assert [pyref.to_raw(v) for v in pyref.xfe_inv(vals)] == inversion_ref.xfe_inv_raw(e.tolist())
    # the vector builder: zeros map to zero under inverse_or_zero and are refused under batch_inversion
    v = oracle.fill_random(30, 0x1AA)
    v[rng.choice(30, 5, replace=False)] = 0
    got = inversion_ref.expected(v, 1)
    assert np.array_equal(got == 0, v == 0)
    with pytest.raises(ZeroDivisionError):
        inversion_ref.expected(v, 1, or_zero=False)
    v3 = oracle.fill_random(30, 0x1AB)
    v3[3:6] = 0
    got3 = inversion_ref.expected(v3, 3)
    assert not got3[3:6].any() and got3[:3].any()


def test_cpp_mirror_inversion_selftest_compiles(tf):
    subprocess.check_call(["make", "-C", HOST, "inversion_selftest"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(HOST, "inversion_selftest"))
    if tf.lib().tf_device_count() == 0:
        r = subprocess.run([os.path.join(HOST, "inversion_selftest")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77, r.stdout + r.stderr
