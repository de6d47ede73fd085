#!/usr/bin/env python3
"""Record what the NTT planner decides into tests/golden/ntt_plans.json (host logic: no device is touched).

For the default setting and for one test hook at a time: tf_ntt_plan over log_n 1..31 x width {1, 3} and tf_ntt_launch_count over
the same grid x batch {1, 64, 4096, 2^22}.  tests/test_abi_and_host.py::test_plans_match_the_recorded_table replays the file, so a
refactoring of the planner cannot move a plan unnoticed; run this again when a plan is changed on purpose.  Record with
TF_NTT_TILE_BYTES and TF_NTT_PIPE unset and with the product library (no TF_HIP_LIBRARY).
"""
import ctypes
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

LOG_N = list(range(1, 32))
WIDTHS = [1, 3]
BATCHES = [1, 64, 4096, 1 << 22]
# (hook, argument, argument that restores the default); tile_bytes 0 = the built-in 2 GiB
SETTINGS = [(None, 0, 0),
            ("tf_set_ntt_min_passes", 3, 0), ("tf_set_ntt_min_passes", 4, 0),
            ("tf_set_ntt_two_pass", 0, -1), ("tf_set_ntt_two_pass", 1, -1), ("tf_set_ntt_two_pass", 3, -1),
            ("tf_set_ntt_small_launch", 0, -1), ("tf_set_ntt_small_launch", 1, -1),
            ("tf_set_ntt_latency_kernel", 0, -1), ("tf_set_ntt_latency_kernel", 1, -1),
            ("tf_set_ntt_tile_bytes", 64 << 20, 0)]


def replay(lib, log_ns, widths, batches):
    """plans[width][log_n] = the radices' log2, one per pass; launches[width][log_n][batch]"""
    radix = (ctypes.c_int * 4)()
    plans, launches = [], []
    for width in widths:
        plans.append([])
        launches.append([])
        for log_n in log_ns:
            passes = lib.tf_ntt_plan(1 << log_n, width, radix)
            plans[-1].append(list(radix)[:passes])
            launches[-1].append([lib.tf_ntt_launch_count(1 << log_n, b, width) for b in batches])
    return plans, launches


def main():
    assert "TF_NTT_TILE_BYTES" not in os.environ and "TF_NTT_PIPE" not in os.environ and "TF_HIP_LIBRARY" not in os.environ
    import twenty_first_amd as tf

    lib = tf.lib()
    table = {"log_n": LOG_N, "widths": WIDTHS, "batches": BATCHES, "settings": []}
    for hook, arg, restore in SETTINGS:
        if hook:
            getattr(lib, hook)(arg)
        try:
            plans, launches = replay(lib, LOG_N, WIDTHS, BATCHES)
        finally:
            if hook:
                getattr(lib, hook)(restore)
        table["settings"].append({"hook": hook, "arg": arg, "restore": restore, "plans": plans, "launches": launches})
    out = os.path.join(ROOT, "tests", "golden", "ntt_plans.json")
    with open(out, "w") as f:
        f.write("{\n")
        for k in ("log_n", "widths", "batches"):
            f.write(f' "{k}": {json.dumps(table[k])},\n')
        f.write(' "settings": [\n')
        f.write(",\n".join("  " + json.dumps(s, separators=(",", ":")) for s in table["settings"]))
        f.write("\n ]\n}\n")
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()
