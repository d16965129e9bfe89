"""Write tests/golden/mnist_launch_args.npz: what the fused MNIST step computes at this commit (training
and evaluation, per batch size), for tests/test_mnist_launch_args_gpu.py to pin bit for bit.

Run once on an MI355X at the commit whose results are the yardstick (before a change to how the kernels
receive their arguments), and commit the output:

    python scripts/make_mnist_launch_args_golden.py

TDL_GOLDEN_ROOT=<dir> takes the built package from <dir> instead of this tree (a snapshot of the
yardstick commit made by scripts/ab_snapshot.sh), with this tree's test module.

See launch_args_record() in the test, which computes both sides."""
import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.abspath(os.environ.get("TDL_GOLDEN_ROOT", ROOT)))


def main():
    spec = importlib.util.spec_from_file_location(
        "launch_args_test", os.path.join(ROOT, "tests", "test_mnist_launch_args_gpu.py"))
    T = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(T)
    print("package:", os.path.dirname(T.M.__file__))
    os.environ.pop("TDL_FX_GRID", None)
    cuda = torch.device("cuda:0")
    out = {}
    for b in T.BATCHES:
        first = T.launch_args_record(cuda, b)
        again = T.launch_args_record(cuda, b)
        for name, v in first.items():
            v = np.asarray(v)
            assert v.tobytes() == np.asarray(again[name]).tobytes(), f"b={b} {name}: not reproducible"
            out[f"b{b}_{name}"] = v
            print(f"b={b} {name}: " + (f"{int(v):#010x}" if v.dtype == np.uint32 else
                                       f"{float(v)}" if v.ndim == 0 else f"{v.size} floats, max |.| {np.abs(v).max():.6g}"))
    os.makedirs(os.path.dirname(T.GOLDEN), exist_ok=True)
    np.savez(T.GOLDEN, **out)
    print(f"wrote {os.path.relpath(T.GOLDEN, ROOT)}: {os.path.getsize(T.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
