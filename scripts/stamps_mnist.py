"""Per-wave phase timestamps (s_memrealtime, 10 ns ticks) of the per-image MNIST kernels.

For every wave slot, prints the median (over workgroups) time from the kernel's first wave start
to each stamped point, so phases of different waves can be compared on one clock."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from tensorflow_distributed_learning_amd.models import mnist_cnn as M  # noqa: E402

KERNELS = {
    "fwd_conv": (8, 8, {0: "start", 1: "stage-issued", 2: "stage-barrier", 3: "conv1-done", 4: "barrier2",
                        5: "conv2-mfma", 6: "dense1-partial", 7: "dP2-done|fused: dP2-start"}, 256),
    "conv_bwd": (6, 8, {0: "start", 1: "stage-issued", 2: "stage-barrier", 3: "wgrad-done", 6: "dgrad-mfma",
                        4: "dgrad-epi", 5: "final-barrier"}, 256),
}


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
    fused = bool(st.fused_bwd)
    print(f"fused_bwd={fused}")
    for name, (k, waves, slots, grid) in KERNELS.items():
        if fused and name == "conv_bwd":
            continue
        # fused kernel: grid * 104 words, then KF-X's (not launched here), then the diagnostics build's
        # "dgrad MFMAs issued" stamp per wave (-DTDL_DIAG_DGRAD_STAMP; zeros in a normal build)
        # then the launch-head stamps of a -DTDL_DIAG_ARGS_STAMP build: the fused kernel's [grid][8][2] =
        # entry, arguments landed; KF-X's [FINALIZE_BLOCKS][8][4] (scripts/stamps_step.py prints those)
        diag0 = grid * 104 + M.FINALIZE_BLOCKS * 16
        args0 = diag0 + grid * 8
        buf = torch.zeros(args0 + grid * 16 + M.FINALIZE_BLOCKS * 32, dtype=torch.int64, device=dev)
        st.forward_backward(0)
        st.finalize(True)
        st._impl.set_stamps(buf)
        st.stage(k)
        st._impl.set_stamps(None)
        torch.cuda.synchronize()
        r = buf[:grid * 64].view(grid, 8, 8).cpu().numpy().astype(np.int64)
        hs = buf[grid * 64:grid * 72].view(grid, 8).cpu().numpy().astype(np.int64)
        t0 = r[:, :waves, 0].min(axis=1, keepdims=True)
        rel = (r - t0[:, :, None]) * 10 / 1000.0  # us since the workgroup's first wave started
        span = (r[:, :waves][r[:, :waves] > 0].max() - r[:, :waves, 0].min()) * 10 / 1000.0
        starts = r[:, 0, 0]
        print(f"{name}: kernel span {span:.2f} us; workgroup start spread {(starts.max() - starts.min()) / 100:.2f} us"
              "  (median us since workgroup start, per wave)")
        if name == "fwd_conv":
            # the loss head ran in the last quarter workgroup of each image: its phases
            # (0 hand-off won, 1 partials loaded, 2 logits/softmax, 3 end) follow the wave stamps
            last = hs[:, 0] > 0
            g0 = r[:, :waves, 0][r[:, :waves, 0] > 0].min()
            h = (hs[last][:, :4] - g0) / 100.0
            p6 = (r[:, 0, 6] - g0) / 100.0
            print(f"  head in {last.sum()} workgroups; us since kernel start (median / max): dense1 partial stored "
                  f"{np.median(p6):.2f}/{p6.max():.2f}; head won {np.median(h[:, 0]):.2f}/{h[:, 0].max():.2f}; "
                  f"partials loaded {np.median(h[:, 1]):.2f}/{h[:, 1].max():.2f}; softmax {np.median(h[:, 2]):.2f}/"
                  f"{h[:, 2].max():.2f}; dH published {np.median(h[:, 3]):.2f}/{h[:, 3].max():.2f}")
            if last.all() and grid % 4 == 0:
                # every quarter ran the head: its wait is set by the LAST of the image's other three
                # quarters to store its partial (p6 of wave 0); loaded - that = visibility + detection
                p6i = p6.reshape(-1, 4)
                other = np.stack([np.delete(p6i, c, axis=1).max(axis=1) for c in range(4)], axis=1).reshape(-1)
                lat = h[:, 1] - other
                polls = hs[:, 4]
                print(f"  partial hand-off: last partner store -> partials loaded median {np.median(lat):.2f} "
                      f"us (p10 {np.percentile(lat, 10):.2f}, p90 {np.percentile(lat, 90):.2f}); poll rounds "
                      f"median {np.median(polls):.0f} (min {polls.min()}, max {polls.max()})")
        if name == "fwd_conv" and fused:
            bs = buf[grid * 72:grid * 104].view(grid, 8, 4).cpu().numpy().astype(np.int64)
            t0w = r[:, :waves, 0].min(axis=1)
            relb = (bs - t0w[:, None, None]) * 10 / 1000.0
            for k2, label in enumerate(["bwd dC2 ready", "bwd wgrad done", "bwd dgrad done", "bwd reduced"]):
                vals = [np.median(relb[:, w, k2]) for w in range(waves)]
                print(f"  {label:14s}" + " ".join(f"{v:6.2f}" for v in vals))
            dg = buf[diag0:args0].view(grid, 8).cpu().numpy().astype(np.int64)
            if (dg > 0).all():
                reld = (dg - t0w[:, None]) * 10 / 1000.0
                print("  bwd dgrad MFMAs" + " ".join(f"{np.median(reld[:, w]):6.2f}" for w in range(waves)))
                # per SIMD (waves s and s + 4): the later wave's last dgrad MFMA -> both waves' dgrad done,
                # i.e. the time the SIMD's MFMA pipe has nothing left but runs the epilogues
                tail = np.maximum(relb[:, :4, 2], relb[:, 4:, 2]) - np.maximum(reld[:, :4], reld[:, 4:])
                print("  exposed dgrad epilogue per SIMD (median / p90 us): " + "  ".join(
                    f"{np.median(tail[:, s]):.2f}/{np.percentile(tail[:, s], 90):.2f}" for s in range(4)))
        if name == "fwd_conv":
            ah = buf[args0:args0 + grid * 16].view(grid, 8, 2).cpu().numpy().astype(np.int64)
            if (ah > 0).all():
                # launch head, on the same clock as the slots below (0 = the workgroup's first "start" stamp,
                # which itself waits for the arguments it reads: the entry is earlier)
                rela = (ah - t0[:, :, None]) * 10 / 1000.0
                print("  entry         " + " ".join(f"{np.median(rela[:, w, 0]):6.2f}" for w in range(waves)))
                print("  args landed   " + " ".join(f"{np.median(rela[:, w, 1]):6.2f}" for w in range(waves)))
                d0 = (ah[:, :, 1] - ah[:, :, 0]) / 100.0
                d1 = (r[:, :waves, 1] - ah[:, :, 1]) / 100.0
                print(f"  launch head (all waves, median / p90 us): entry -> args landed {np.median(d0):.2f}/"
                      f"{np.percentile(d0, 90):.2f}; args landed -> stage-issued {np.median(d1):.2f}/"
                      f"{np.percentile(d1, 90):.2f}; entry -> stage-issued {np.median(d0 + d1):.2f}/"
                      f"{np.percentile(d0 + d1, 90):.2f}")
        print("  slot/wave " + " ".join(f"{w:>6d}" for w in range(waves)))
        for s, label in sorted(slots.items(), key=lambda kv: np.median(rel[:, 0, kv[0]])):
            vals = [np.median(rel[:, w, s]) if (r[:, w, s] > 0).all() else float("nan") for w in range(waves)]
            print(f"  {label:14s}" + " ".join(f"{v:6.2f}" for v in vals))


if __name__ == "__main__":
    main()
