"""Write tests/golden/mnist_fused_bwd.npz: what the fused MNIST step's backward computes at this
commit, for tests/test_mnist_fused_bwd_golden_gpu.py to pin bit for bit.

Run once on an MI355X at the commit whose results are the yardstick (before a change that must not
move a bit), and commit the output:

    python scripts/make_mnist_golden.py

Per batch size it stores dW1 / db1 raw (320 floats) and CRC-32s of dW2, db2, the whole gradient slab
and the weights after three SGD steps -- see golden_record() in the test, which computes both sides."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    spec = importlib.util.spec_from_file_location(
        "golden_test", os.path.join(ROOT, "tests", "test_mnist_fused_bwd_golden_gpu.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    cuda = torch.device("cuda:0")
    out = {}
    for b in T.GOLDEN_BATCHES:
        first = T.golden_record(cuda, b)
        again = T.golden_record(cuda, b)
        for name, v in first.items():
            assert np.array_equal(np.asarray(v), np.asarray(again[name])), f"b={b} {name}: not reproducible"
            out[f"b{b}_{name}"] = v
            print(f"b={b} {name}: " + (f"{int(v):#010x}" if np.ndim(v) == 0 else f"{v.size} floats, max |.| {np.abs(v).max():.6g}"))
    os.makedirs(os.path.dirname(T.GOLDEN), exist_ok=True)
    np.savez(T.GOLDEN, **out)
    print(f"wrote {os.path.relpath(T.GOLDEN, ROOT)}: {os.path.getsize(T.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
