"""The guard mode for library-owned device memory (tf_debug_temp_guard), as far as a machine without a GPU can check it:

  * closure: every allocation site of csrc/ -- .alloc(, .alloc_bytes(, .put(, pool_malloc_async(, scratch_acquire( and the three
    helpers that forward a label to one of them -- carries a literal label, and the set of labels in the source is exactly the
    union of the labels the GPU cases of tests/test_gpu_temp_guard.py declare they must see.  There is no exemption list: a new
    allocation site without a guarded GPU case fails here;
  * the header's constant equals fence.G, and its poison sequence equals fence.poison_words on its first words (compiled with the
    host compiler alone: csrc/tf_temp_guard.h is plain C++ there).

The counterpart of tests/test_fence_cpu.py; the device side of the mechanism proves itself in test_gpu_temp_guard.py (the self-test)."""
import glob
import os
import re
import subprocess

import numpy as np

from tests import fence

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "twenty-first_amd", "csrc")
# the allocation calls, and the helpers that take a label and hand it on to one of them (their call sites are sites too)
SITES = (".alloc(", ".alloc_bytes(", ".put(", "pool_malloc_async(", "scratch_acquire(")
FORWARDERS = ("up_words(", ".get(&")   # (WorkSpace::get(&pointer, words, label) of tf_divide.hip, whatever the work space is called)
STRING = re.compile(r'"(?:[^"\\\n]|\\.)*"')


def _blank(m):
    return '"' + "_" * (len(m.group(0)) - 2) + '"'


def sites():
    """(file, line, label or None) of every allocation site; None for a site that only forwards its caller's `what`"""
    found = []
    for path in sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h"))):
        text = open(path).read()
        text = re.sub(r"//[^\n]*", lambda m: " " * len(m.group(0)), STRING.sub(lambda m: m.group(0).replace("//", "__"), text))   # comments out, strings kept
        masked = STRING.sub(_blank, text)                                # what sits inside a string is no call
        for pattern in SITES + FORWARDERS:
            at = masked.find(pattern)
            while at >= 0:
                start = at + len(pattern)
                depth, j = 1, start
                while depth:
                    depth += {"(": 1, ")": -1}.get(masked[j], 0)
                    j += 1
                args, line = text[start:j - 1], text.count("\n", 0, at) + 1
                literals = [m.group(0)[1:-1] for m in STRING.finditer(args)]
                name = os.path.basename(path)
                if len(literals) == 1:
                    found.append((name, line, literals[0]))
                elif not literals and re.search(r"\bwhat\b", args):
                    found.append((name, line, None))                     # a definition, a declaration or a forwarding call
                else:
                    raise AssertionError(f"{name}:{line}: {pattern}{args.strip()}) carries no literal label")
                at = masked.find(pattern, j)
    return found


def test_every_allocation_site_carries_a_literal_label():
    found = sites()
    labelled = [s for s in found if s[2] is not None]
    assert len(labelled) >= 90, len(labelled)
    assert all(label.strip() == label and label for _, _, label in labelled)
    # the sites that only forward: the definitions / declarations of the five functions and of the helpers, and the helpers' own inner calls
    assert {f for f, _, label in found if label is None} <= {"tf_temp.h", "tf_internal.h", "tf_ntt.hip", "tf_mmr.hip", "tf_divide.hip", "tf_points.hip"}


def test_labels_in_the_source_are_exactly_the_labels_the_gpu_cases_declare():
    from tests import test_gpu_temp_guard as g

    in_source = {label for _, _, label in sites() if label is not None}
    declared = set(g.host_labels()) | set(g.CACHE_LABELS)
    for labels in g.WITNESS.values():
        declared |= set(labels)
    assert in_source - declared == set(), f"allocation sites no guarded GPU case must see: {sorted(in_source - declared)}"
    assert declared - in_source == set(), f"declared labels that no allocation site carries: {sorted(declared - in_source)}"
    # every witness names a case that exists
    for (src, name, k) in g.WITNESS:
        assert 0 <= k < len(g.SOURCES[src].ROWS[name][0]), (src, name, k)


def test_header_constant_and_poison_sequence_match_the_fence(tmp_path):
    src = tmp_path / "poison.cpp"
    src.write_text('#include <cstdio>\n#include "tf_temp_guard.h"\nint main() {\n  std::printf("%zu %d\\n", tfi::kTempGuardWords, (int)tfi::kTempGuardLedgerWords);\n'
                   '  for (int mode = 1; mode <= 3; ++mode)\n    for (unsigned long long i = (mode == 3 ? 20470 : 0), e = i + 64; i < e; ++i)\n'
                   '      std::printf("%llu %u %u\\n", (unsigned long long)tfi::temp_guard_poison(mode, i),\n'
                   '                  tfi::temp_guard_poison32(mode, 2 * i), tfi::temp_guard_poison32(mode, 2 * i + 1));\n  return 0;\n}\n')
    exe = tmp_path / "poison"
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-I", CSRC, "-o", str(exe), str(src)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    g, ledger = (int(v) for v in lines[0].split())
    assert g == fence.G and ledger == fence.LEDGER_WORDS
    header = open(os.path.join(ROOT, "include", "tf_hip.h")).read()
    assert f"TF_TEMP_GUARD_WORDS = {fence.G}," in header and f"TF_TEMP_GUARD_LEDGER_WORDS = {fence.LEDGER_WORDS} " in header
    rows = np.array([[int(v) for v in l.split()] for l in lines[1:1 + 3 * 64]], dtype=np.uint64).reshape(3, 64, 3)
    for m, kind in enumerate(fence.POISONS):
        first = 20470 if kind == "random" else 0     # (the random words straddle the end of the front guard)
        want = fence.poison_words(kind, first + 64)[first:]
        assert np.array_equal(rows[m, :, 0], want), kind
        assert np.array_equal(rows[m, :, 1], want & np.uint64(0xFFFFFFFF)) and np.array_equal(rows[m, :, 2], want >> np.uint64(32)), kind
