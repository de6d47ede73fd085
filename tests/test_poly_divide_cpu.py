"""Division with remainder and the power-series inverse (Polynomial::divide / reduce / Div / Rem and
formal_power_series_inverse_newton, math/polynomial.rs:539-600, :989-1048, :1281-1366, :2502-2524): the parts that need no GPU --
the exported symbols, the argument errors every flavour returns before any HIP call, the length of the Newton iterate and the C++
mirror's self-test program."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HOST = os.path.join(ROOT, "twenty-first_amd", "host")

NEW = ("tf_poly_divide_bfe", "tf_poly_divide_xfe", "tf_poly_divide_bfe_dev", "tf_poly_divide_xfe_dev",
       "tf_poly_fps_inverse_newton_bfe", "tf_poly_fps_inverse_newton_xfe", "tf_poly_fps_inverse_newton_bfe_dev",
       "tf_poly_fps_inverse_newton_xfe_dev", "tf_poly_fps_inverse_newton_len")
OK, NULL, TOO_LARGE, INVERSE_OF_ZERO, DIV_ZERO, INVALID = 0, 7, 5, 12, 15, 17


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
    a = np.ones(8 * w, dtype=np.uint64)
    b = np.ones(3 * w, dtype=np.uint64)
    q = np.zeros(6 * w, dtype=np.uint64)
    r = np.zeros(2 * w, dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    host = getattr(lib, f"tf_poly_divide_{suffix}")
    dev = getattr(lib, f"tf_poly_divide_{suffix}_dev")
    # nb == 0: the reference's "divisor should be non-zero" panic
    assert host(_p(a), 8, 1, _p(b), 0, _p(q), _p(r)) == DIV_ZERO
    assert dev(_p(a), 8, 1, _p(b), 0, _p(q), _p(r), None, _p(st)) == DIV_ZERO
    # both outputs NULL
    assert host(_p(a), 8, 1, _p(b), 3, None, None) == NULL
    assert dev(_p(a), 8, 1, _p(b), 3, None, None, None, _p(st)) == NULL
    # NULL d_status
    assert dev(_p(a), 8, 1, _p(b), 3, _p(q), _p(r), None, None) == NULL
    # NULL operands, limits
    assert host(None, 8, 1, _p(b), 3, _p(q), None) == NULL
    assert host(_p(a), 8, 1, None, 3, None, _p(r)) == NULL
    assert host(_p(a), 8, 65536, _p(b), 3, _p(q), _p(r)) == TOO_LARGE
    assert dev(_p(a), (1 << 30) + 1, 1, _p(b), 3, _p(q), _p(r), None, _p(st)) == TOO_LARGE
    # an unnormalised divisor is the host form's return value (the _dev form reports it through d_status)
    b0 = b.copy()
    b0[2 * w:] = 0
    assert host(_p(a), 8, 1, _p(b0), 3, _p(q), _p(r)) == INVALID
    # nothing to do
    assert host(_p(a), 8, 0, _p(b), 3, _p(q), _p(r)) == OK
    assert dev(_p(a), 8, 0, _p(b), 3, _p(q), _p(r), None, _p(st)) == OK


@pytest.mark.parametrize("suffix", ["bfe", "xfe"])
def test_fps_argument_errors_without_device(tf, suffix):
    lib = tf.lib()
    w = 1 if suffix == "bfe" else 3
    f = np.ones(4 * w, dtype=np.uint64)
    out = np.zeros(64 * w, dtype=np.uint64)
    st = np.zeros(1, dtype=np.int32)
    host = getattr(lib, f"tf_poly_fps_inverse_newton_{suffix}")
    dev = getattr(lib, f"tf_poly_fps_inverse_newton_{suffix}_dev")
    assert host(_p(f), 0, 8, _p(out)) == INVERSE_OF_ZERO
    assert dev(_p(f), 0, 8, _p(out), None, _p(st)) == INVERSE_OF_ZERO
    f0 = f.copy()
    f0[:w] = 0
    assert host(_p(f0), 4, 8, _p(out)) == INVERSE_OF_ZERO
    f1 = f.copy()
    f1[3 * w:] = 0
    assert host(_p(f1), 4, 8, _p(out)) == INVALID
    assert host(_p(f), 4, 8, None) == NULL
    assert dev(_p(f), 4, 8, _p(out), None, None) == NULL
    assert host(_p(f), 4, 1 << 40, _p(out)) == TOO_LARGE
    # sized from tf_poly_fps_inverse_newton_len (0 in both cases), a NULL output still gets the panic code / the size limit
    assert host(None, 0, 8, None) == INVERSE_OF_ZERO
    assert dev(None, 0, 8, None, None, _p(st)) == INVERSE_OF_ZERO
    assert host(_p(f), 4, 1 << 40, None) == TOO_LARGE


def _len_by_recurrence(nf, precision):
    d = nf - 1
    if d == 0:
        return 1
    rounds = max(precision, 1)
    rounds = (1 << (rounds - 1).bit_length()).bit_length() - 1  # ilog2(next_power_of_two(precision)), 0 counted as 1
    deg = 0
    for _ in range(rounds):
        deg = 2 * deg + d  # f_(i+1) = 2 f_i - f_i^2 g
    return deg + 1


def test_fps_len_matches_the_recurrence(tf):
    n = tf.lib().tf_poly_fps_inverse_newton_len
    for nf in (1, 2, 4, 256, 257, 258, 1001):
        for precision in (0, 1, 2, 3, 8, 9, 1024, 1025):
            assert n(nf, precision) == _len_by_recurrence(nf, precision), (nf, precision)
    assert n(0, 8) == 0
    assert n(2, 1 << 31) == 0  # 2^31 coefficients: above the 2^30 limit
    assert n(2, 1 << 30) == (1 << 30)


def test_python_shapes_are_checked_on_the_host(tf):
    with pytest.raises(tf.NttPanic) as e:
        tf.poly_divide(np.ones(4, dtype=np.uint64), np.zeros(2, dtype=np.uint64))
    assert e.value.code == DIV_ZERO
    with pytest.raises(ValueError):
        tf.poly_divide(np.ones(5, dtype=np.uint64), np.ones(2, dtype=np.uint64), batch=2)


def test_cpp_mirror_divide_selftest_compiles(tf):
    subprocess.check_call(["make", "-C", HOST, "divide_selftest"], stdout=subprocess.DEVNULL)
    assert os.path.exists(os.path.join(HOST, "divide_selftest"))
    if tf.lib().tf_device_count() == 0:
        r = subprocess.run([os.path.join(HOST, "divide_selftest")], capture_output=True, text=True, timeout=120)
        assert r.returncode == 77, r.stdout + r.stderr
