"""Whole-step timeline of the fused MNIST step (fused kernel + KF-X finalize) from per-wave
s_memrealtime stamps (10 ns ticks): span of each launch and the gap between them."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorflow_distributed_learning_amd.models import mnist_cnn as M  # noqa: E402


def _cats(nfx):
    """KF-X block ranges (dW3 / small dense / conv2 / conv1) for a finalize of nfx workgroups."""
    d = nfx - 146 - 20  # kFxDense (= kFxW3 + 9 small dense blocks)
    return {f"dW3 rows (0-{d - 10})": (0, d - 9), f"db3/dW4/db4 ({d - 9}-{d - 1})": (d - 9, d),
            f"conv2 pieces ({d}-{d + 145})": (d, d + 146), f"conv1 ({d + 146}-{nfx - 1})": (d + 146, nfx)}


def main():
    dev = torch.device("cuda:0")
    b, N = 64, 60000
    X = torch.rand(N, 28, 28, 1, device=dev)
    Y = torch.randint(0, 10, (N,), device=dev, dtype=torch.int32)
    layout = M.mnist_layout()
    W = layout.pack(M.init_mnist_params(0), device=dev)
    G = torch.zeros_like(W)
    idx = torch.randperm(N, device=dev)[:b].to(torch.int32)
    lr = torch.tensor([1e-3], device=dev)
    st = M.FusedMnistTrainStep(X, Y, idx, W, G, layout, b, 1, lr)
    for _ in range(20):
        st.forward_backward(0)
        st.finalize(True)
    grid, nfx = 4 * b, M.FINALIZE_BLOCKS
    CATS = _cats(nfx)
    rows, cats, lasts, heads, fheads = [], [], [], [], []
    for rep in range(int(os.environ.get("REPS", "20"))):
        # (+ grid * 8 words: a -DTDL_DIAG_DGRAD_STAMP build stamps there, see stamps_mnist.py)
        # (+ grid * 16 + nfx * 32 words: the launch-head stamps of a -DTDL_DIAG_ARGS_STAMP build -- the fused
        # kernel's [grid][8][2] = entry, arguments landed; KF-X's [nfx][8][4] = entry, arguments landed, first
        # operand load about to issue)
        args0 = grid * 104 + nfx * 16 + grid * 8
        buf = torch.zeros(args0 + grid * 16 + nfx * 32, dtype=torch.int64, device=dev)
        st._impl.set_stamps(buf)
        st.forward_backward(0)
        st.finalize(True)
        st._impl.set_stamps(None)
        torch.cuda.synchronize()
        f = buf[:grid * 104].cpu().numpy().astype(np.int64)
        f = f[f > (1 << 32)]  # (time stamps only: the head's slot 4 holds a poll count)
        x = buf[grid * 104:grid * 104 + nfx * 16].view(nfx, 8, 2).cpu().numpy().astype(np.int64)
        t0 = f.min()
        fa = buf[args0:args0 + grid * 16].view(grid, 8, 2).cpu().numpy().astype(np.int64)
        xa = buf[args0 + grid * 16:].view(nfx, 8, 4).cpu().numpy().astype(np.int64)
        if (fa[:, :, 0] > 0).all():
            st1 = buf[:grid * 64].view(grid, 8, 8)[:, :, 1].cpu().numpy().astype(np.int64)  # stage-issued
            fheads.append([np.median(fa[:, :, 1] - fa[:, :, 0]) / 100 if (fa[:, :, 1] > 0).all() else np.nan,
                           np.median(st1 - fa[:, :, 0]) / 100])
            hk = []
            for nm, (lo, hi) in CATS.items():
                nw = 4 if nm.startswith("dW3") else 2 if nm.startswith("db3") else 8  # waves with a task
                e, l, o, end = xa[lo:hi, :nw, 0], xa[lo:hi, :nw, 1], xa[lo:hi, :nw, 2], x[lo:hi, :nw, 1]
                busy = o > 0
                hk.append([np.median((l - e)[l > 0]) / 100 if (l > 0).any() else np.nan,
                           np.median((o - e)[busy]) / 100, np.median((end - e)[busy]) / 100])
            heads.append(hk)
        xs0 = x[:, :, 0].min()
        cats.append([((x[lo:hi, :, 0].min() - xs0) / 100, (np.median(x[lo:hi, :, 0]) - xs0) / 100,
                      (np.median(x[lo:hi, :, 1]) - xs0) / 100, (x[lo:hi, :, 1].max() - xs0) / 100)
                     for lo, hi in CATS.values()])
        lasts.append((x[:, :, 1].max(axis=1) - xs0) / 100)  # per-block last wave end
        rows.append([(f.max() - t0) / 100, (x[:, :, 0].min() - f.max()) / 100, (x[:, :, 1].max() - x[:, :, 0].min()) / 100,
                     (np.median(x[:, :, 1] - x[:, :, 0])) / 100, (x[:, :, 0].max() - x[:, :, 0].min()) / 100,
                     (x[:, :, 1].max() - t0) / 100])
        for _ in range(3):
            st.forward_backward(0)
            st.finalize(True)
    a = np.array(rows)
    names = ["fused span", "gap fused->KF-X", "KF-X span", "KF-X median wave life", "KF-X wave start spread", "step span"]
    for k, nm in enumerate(names):
        print(f"{nm:24s} median {np.median(a[:, k]):6.2f} us  min {a[:, k].min():6.2f}  max {a[:, k].max():6.2f}")
    c = np.median(np.array(cats), axis=0)
    print("KF-X blocks, us since KF-X first wave (median over reps): first start / median start / median end / last end")
    for (nm, _), v in zip(CATS.items(), c):
        print(f"  {nm:22s} " + " ".join(f"{t:6.2f}" for t in v))
    if fheads:
        fh = np.median(np.array(fheads), axis=0)
        print(f"launch head, fused kernel (median over waves and reps, us): entry -> args landed {fh[0]:.2f}; "
              f"entry -> stage-issued {fh[1]:.2f}")
        print("launch head, KF-X per range kind (busy waves): entry -> args landed / entry -> first operand load / "
              "entry -> wave end")
        for (nm, _), v in zip(CATS.items(), np.median(np.array(heads), axis=0)):
            print(f"  {nm:22s} " + " ".join(f"{t:6.2f}" for t in v))
    ml = np.median(np.array(lasts), axis=0)
    late = np.argsort(ml)[::-1][:12]
    print("latest KF-X blocks (median last-wave end, us): " + ", ".join(f"{j}:{ml[j]:.2f}" for j in late))


if __name__ == "__main__":
    main()
