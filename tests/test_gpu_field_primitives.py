"""Every hand-scheduled field primitive (csrc/gl64.h: add_sub, add_sub2, add_sub_lazy2, add_lazy4, sub_lazy4, mont_mul2/3/4,
canonical_asm; csrc/tip5_kernels.h: mx_fold4_tail<CANON>, mx_fold2_tail; and the compiler forms gl::add, gl::sub, gl::mont_mul) against
Python integers, on operands that take the carry paths uniform words take once in 2^32 pairs.

tf_debug_field_op_dev runs ONE primitive over an array of operand pairs, W consecutive elements per thread, through the very function
the kernels call.  tests/field_ref.py holds the operand sets (edge words' cross product, 2^16 uniform pairs, pairs built backwards
from results on a carry path; every pair at every block position) and the expected words; tests/test_field_primitives_cpu.py checks
that every path is reached at least eight times per position.
"""
import numpy as np
import pytest

from tests import field_ref as ref

pytestmark = pytest.mark.gpu

GUARD = 64  # canary words behind each output
CANARY = 0xA5A5A5A5A5A5A5A5
THREADS = 256  # per workgroup: one workgroup's worth of elements is THREADS * W


@pytest.fixture(scope="module", autouse=True)
def _need_gpu(tf):
    assert tf.lib().tf_device_count() > 0, "no HIP device visible: the product has no CPU fallback"


def _u64(words):
    return np.array(words, dtype=np.uint64)


def _run(tf, op, a, b):
    """one call on a[:], b[:] -> (out0, out1 or None) as uint64 arrays, after checking the canaries behind both outputs"""
    import torch

    n = len(a)
    canary = np.full(GUARD, CANARY, dtype=np.uint64)
    fresh = np.concatenate([np.full(n, 0x5A5A5A5A5A5A5A5A, dtype=np.uint64), canary]).view(np.int64)
    da, db = torch.from_numpy(a.view(np.int64)).cuda(), torch.from_numpy(b.view(np.int64)).cuda()
    outs = [torch.from_numpy(fresh.copy()).cuda() for _ in range(ref.outputs(op))]
    tf.device.debug_field_op(op, da, db, outs[0][:n], outs[1][:n] if len(outs) == 2 else None)
    torch.cuda.synchronize()
    got = [o.cpu().numpy().view(np.uint64) for o in outs]
    for k, g in enumerate(got):
        assert np.array_equal(g[n:], canary), f"{op}: words behind out{k} were written (count {n})"
    return [g[:n] for g in got] + [None] * (2 - len(got))


def _compare(op, a, b, got, want, out):
    bad = np.nonzero(got != want)[0]
    if bad.size:
        j = int(bad[0])
        pos = j % ref.width(op)
        raise AssertionError(f"{op} out{out}: {bad.size} of {len(a)} words differ; first at element {j}, chain position {pos} "
                             f"({ref.event(op, out, pos, int(a[j]), int(b[j]))[0]}): a = {int(a[j]):#018x}, b = {int(b[j]):#018x}, "
                             f"got {int(got[j]):#018x}, want {int(want[j]):#018x}; positions hit: {sorted(set(int(i) % ref.width(op) for i in bad))}")


@pytest.mark.parametrize("op", list(ref.OPS))
def test_primitive_on_every_carry_path(tf, op):
    """the whole operand set of the op, every pair at every block position, in one call"""
    a, b, want0, want1, _ = ref.uploaded(op)
    a, b = _u64(a), _u64(b)
    got0, got1 = _run(tf, op, a, b)
    _compare(op, a, b, got0, _u64(want0), 0)
    if want1 is not None:
        _compare(op, a, b, got1, _u64(want1), 1)


@pytest.mark.parametrize("op", list(ref.OPS))
def test_ragged_counts(tf, op):
    """counts around a thread's W elements and around one workgroup's worth: partial blocks compute with zeros for the missing
    operands and store nothing behind count"""
    w = ref.width(op)
    a_all, b_all, want0, want1, _ = ref.uploaded(op)
    for count in sorted({1, w - 1, w, w + 1, THREADS * w - 1, THREADS * w + 1} - {0}):
        a, b = _u64(a_all[:count]), _u64(b_all[:count])
        got0, got1 = _run(tf, op, a, b)
        _compare(op, a, b, got0, _u64(want0[:count]), 0)
        if want1 is not None:
            _compare(op, a, b, got1, _u64(want1[:count]), 1)
