"""Time of forward + backward of tools_for_model.stft and tools_for_model.istft against torch.stft / torch.istft autograd on the same device.
For information only: there is no bar (the commit before could not run a backward at all, and nobody had measured torch's).

    python tools/torchstft_bench.py [--out profiles/torchstft_bench.json]

B = 32 clips of 48000 samples, fp32, at n_fft / hop / win = 512 / 256 / 512 and at the reference's FullSubNet defaults 512 / 300 / 400
(hop_length = int(400 * 0.75)).  One measurement is the public call with an input that requires a gradient plus torch.autograd.grad of a fixed
cotangent, between two device events (host-side launch work of both arms included: this is what a training step pays); 20 warm-ups, then 200 runs
per arm, the arms alternating; medians.  The per-op medians of the two adjoint plans (Plan.run_timed, 50 runs) are reported beside them."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OP_NAMES = {16: "OLA_BWD", 18: "SPECOUT_BWD", 37: "STFT_FFT", 39: "ISTFT_FFT", 52: "OLA_FOLD", 53: "SPECOUT_ADJ"}
GEOMETRIES = ((512, 256, 512), (512, 300, 400))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "torchstft_bench.json"))
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--samples", type=int, default=48000)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--runs", type=int, default=200)
    a = ap.parse_args()
    import sefd_amd  # noqa: F401
    from sefd_amd import tools_for_model as tools
    from sefd_amd.plan import PHASE_FWD, Plan

    dev = torch.device("cuda:0")
    gen = torch.Generator().manual_seed(1)
    B, L = a.batch, a.samples
    cases = {}
    for nfft, hop, win in GEOMETRIES:
        T = 1 + L // hop
        x = (torch.randn(B, L, generator=gen) * 0.3).to(dev)
        w = torch.hann_window(win, device=dev)
        S = torch.stft(x, nfft, hop, win, window=w, return_complex=True)
        g_spec = torch.view_as_complex(torch.randn(B, nfft // 2 + 1, T, 2, generator=gen)).to(dev)
        g_wav = torch.randn(B, L, generator=gen).to(dev)
        geo = f"{nfft}/{hop}/{win}"

        def stft_ours(x=x, g=g_spec, q=(nfft, hop, win)):
            xx = x.detach().requires_grad_(True)
            return torch.autograd.grad(tools.stft(xx, *q), xx, g)[0]

        def stft_torch(x=x, g=g_spec, q=(nfft, hop, win), w=w):
            xx = x.detach().requires_grad_(True)
            return torch.autograd.grad(torch.stft(xx, *q, window=w, return_complex=True), xx, g)[0]

        def istft_ours(S=S, g=g_wav, q=(nfft, hop, win)):
            ss = S.detach().requires_grad_(True)
            return torch.autograd.grad(tools.istft(ss, *q, length=L), ss, g)[0]

        def istft_torch(S=S, g=g_wav, q=(nfft, hop, win), w=w):
            ss = S.detach().requires_grad_(True)
            return torch.autograd.grad(torch.istft(ss, *q, window=w, length=L), ss, g)[0]

        cases[("stft", geo)] = dict(sefd=stft_ours, torch=stft_torch)
        cases[("istft", geo)] = dict(sefd=istft_ours, torch=istft_torch)

    def run(fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1)

    ms = {(k, arm): [] for k in cases for arm in ("sefd", "torch")}
    for i in range(a.warmup + a.runs):
        for k, fns in cases.items():
            for arm in ("sefd", "torch"):
                t = run(fns[arm])
                if i >= a.warmup:
                    ms[(k, arm)].append(t)
    rec = dict(shape=dict(B=B, L=L), dtype="fp32", warmup=a.warmup, runs=a.runs, device=torch.cuda.get_device_name(0), torch=torch.__version__,
               what="forward + backward through the public call, device events, medians, arms alternating; no bar", fwd_bwd={}, adjoint_ops={})
    for (name, geo), _ in cases.items():
        s, t = ms[((name, geo), "sefd")], ms[((name, geo), "torch")]
        rec["fwd_bwd"][f"{name} {geo}"] = dict(sefd_ms_median=round(statistics.median(s), 5), sefd_ms_min=round(min(s), 5),
                                               torch_ms_median=round(statistics.median(t), 5), torch_ms_min=round(min(t), 5))
    stream = torch.cuda.current_stream().cuda_stream
    for nfft, hop, win in GEOMETRIES:
        for model in ("TorchSTFTAdj", "TorchISTFTAdj"):
            plan = Plan(B, L, win_len=win, win_inc=hop, fft_len=nfft, model=model)
            ar = plan.alloc_arenas(dev)
            io = ar[5].view(torch.float32)
            io.copy_((torch.rand(io.numel(), generator=gen) - 0.5).to(dev))
            kinds = [int(k) for k in plan.op_kinds(PHASE_FWD)[0]]
            per = [plan.run_timed(PHASE_FWD, ar, stream) for _ in range(50)]
            rec["adjoint_ops"][f"{model} {nfft}/{hop}/{win}"] = {OP_NAMES.get(k, str(k)): round(statistics.median(p[i] for p in per), 5) for i, k in enumerate(kinds)}
    print(json.dumps(rec))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(rec, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
