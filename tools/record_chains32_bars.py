"""Record tests/golden/chains32_bars.json: for every backward case of tests/chains32.py the kink reach KINK32, the seed of its inputs
and the gradient bars, per tensor and per batch row (`chains32.measure`: the float32 stand-in against the float64 oracle over
`links16.STANDIN_SEEDS` seeds, one thread).  CPU only:

    python tools/record_chains32_bars.py

tests/test_chains32_cpu.py recomputes and re-asserts every entry.

TEST INFRASTRUCTURE: not imported by the product.
"""
import json
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
for p in ("tests", "oracle", "benchmarking-lvms_amd"):
    sys.path.insert(0, os.path.join(ROOT, p))

import chains32 as C  # noqa: E402

if __name__ == "__main__":
    table = {}
    for ct in C.BWD_CASES:
        e = C.measure(ct)
        table[C.case_id(ct)] = {k: e[k] for k in ("kink32", "seed", "bars", "row_bars")}
        near = C.inputs(ct[0], ct[1], e["seed"], e["kink32"])[0]["near_kink"]
        print(f"{C.case_id(ct)}: kink32 {e['kink32']:.1e}, seed {e['seed']}, {int(near.sum())} of {near.numel()} rows left out, "
              f"stand-in worst tensor {max(e['floor'].values()):.2e}, worst batch row {max(e['row_floor'].values()):.2e}, "
              f"largest bar {max(list(e['bars'].values()) + list(e['row_bars'].values())):.1e}")  # fmt: skip
    with open(C.BARS_FILE, "w") as f:
        json.dump(table, f, indent=0, sort_keys=True)
