"""Record what heapdict 1.0.1 itself pops, for tests/test_hastar_cpu.py.

    python tests/golden/make_heapdict_golden.py [path/to/heapdict.py]

Needs the heapdict package (1.0.1, the version the reference's hybrid A* runs on) importable, or the path of
its one module.  Replays the test's seeded operation sequence (heapdict_ops below: inserts and decrease/increase
-key with many priority ties, popitem in between, drain at the end) on heapdict.heapdict and stores every popped
(key, priority) pair in order as heapdict_1_0_1_pops.npz -- data only, no source is copied.
"""
import importlib.util
import os
import random
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
PATH = os.path.join(HERE, "heapdict_1_0_1_pops.npz")
TRIALS, OPS, SEED = 40, 300, 5


def heapdict_ops(make):
    """The operation sequence on a fresh `make()` per trial; yields every popitem() result."""
    rnd = random.Random(SEED)
    for _ in range(TRIALS):
        h = make()
        for _ in range(OPS):
            op = rnd.random()
            if op < 0.6 or len(h) == 0:
                k = rnd.randrange(40)
                h[k] = float(rnd.choice([1, 2, 2, 3, 3, 3, 4.5, 5]))  # many ties
            else:
                yield h.popitem()
        while len(h):
            yield h.popitem()


def main():
    if len(sys.argv) > 1:
        spec = importlib.util.spec_from_file_location("heapdict_ref", sys.argv[1])
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
    else:
        import heapdict as mod
    pops = list(heapdict_ops(mod.heapdict))
    np.savez_compressed(PATH, keys=np.array([k for k, _ in pops], np.int32),
                        priorities=np.array([v for _, v in pops], np.float64))
    print("wrote", PATH, len(pops), "pops")


if __name__ == "__main__":
    main()
