"""The S3IM loss (neuralsim_amd/losses.py ``s3im_loss``, kernels ``nsim_ssim_*``) at the reference's defaults: 4096 rays, 64 x 64
patch, ``repeat_time`` 10, ``kernel_size`` = ``stride`` = 4.

1. One forward + backward pair (index drawn outside the timing) with the HIP functions, beside the same formula in torch ops on the
   device -- gather, five grouped ``conv2d``, the elementwise SSIM map, autograd's backward: what ``S3IMLoss`` over the pytorch-ssim
   form runs.  Per variant: the median of the host clock around a synchronised pair and of the HIP events around it, after
   ``--warmup`` pairs, and what one pair issues (C-ABI calls and ATen operator calls, counted once outside the timing).
2. The headline ``RenderTrainer`` step of bench.py (``build_trainer``) in three modes: ``fused`` (the default launch chain, no S3IM),
   ``autograd`` (the generic path the term needs, still without it) and ``s3im`` (``w_s3im`` > 0).  Blocks of ``--block`` steps
   timed with one synchronisation at the end of a block (``host`` = the part of it the host spent issuing the steps), the modes
   alternated ``--rounds`` times in one process, medians over the blocks.

Prints one JSON line.

    python tools/s3im_bench.py [--rays 4096] [--repeats 50] [--warmup 10] [--out profiles/s3im_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def torch_s3im(pred, gt, index, patch_hw, k, s):
    """1 - SSIM of the virtual images in torch ops (f32, on the tensors' device), the conv2d form"""
    import torch
    import torch.nn.functional as F
    ph, pw = patch_hw
    P = ph * pw
    i = torch.arange(k, dtype=torch.float32, device=pred.device)
    g = torch.exp(-(i - k // 2) ** 2 / (2.0 * 1.5 ** 2))
    g = g / g.sum()
    w = (g[:, None] * g[None, :]).expand(3, 1, k, k).contiguous()
    x = pred[:P][index].permute(1, 0).reshape(1, 3, ph, -1)
    y = gt[:P][index].permute(1, 0).reshape(1, 3, ph, -1)
    p = (k - 1) // 2
    mu1, mu2 = F.conv2d(x, w, padding=p, stride=s, groups=3), F.conv2d(y, w, padding=p, stride=s, groups=3)
    mu1_sq, mu2_sq, mu12 = mu1 * mu1, mu2 * mu2, mu1 * mu2
    s11 = F.conv2d(x * x, w, padding=p, stride=s, groups=3) - mu1_sq
    s22 = F.conv2d(y * y, w, padding=p, stride=s, groups=3) - mu2_sq
    s12 = F.conv2d(x * y, w, padding=p, stride=s, groups=3) - mu12
    C1, C2 = 0.01 ** 2, 0.03 ** 2
    m = ((2 * mu12 + C1) * (2 * s12 + C2)) / ((mu1_sq + mu2_sq + C1) * (s11 + s22 + C2))
    return 1.0 - m.mean()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=4096)
    ap.add_argument("--patch", type=int, nargs=2, default=[64, 64])
    ap.add_argument("--repeat-time", type=int, default=10)
    ap.add_argument("--kernel-size", type=int, default=4)
    ap.add_argument("--stride", type=int, default=4)
    ap.add_argument("--w", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--block", type=int, default=20)
    ap.add_argument("--blocks", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--no-step", action="store_true", help="skip part 2")
    ap.add_argument("--out", type=str, default=None)
    args = ap.parse_args()
    import torch
    from torch.utils._python_dispatch import TorchDispatchMode
    from neuralsim_amd import _lib, losses
    assert torch.cuda.is_available(), "s3im_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    N, hw, R, k, s = args.rays, tuple(args.patch), args.repeat_time, args.kernel_size, args.stride
    gen = torch.Generator(device=dev).manual_seed(1)
    pred0, gt = torch.rand([N, 3], device=dev, generator=gen), torch.rand([N, 3], device=dev, generator=gen)
    index = losses.s3im_index(hw[0] * hw[1], R, dev, generator=gen)

    class Count(TorchDispatchMode):
        n = 0

        def __torch_dispatch__(self, func, types, args=(), kwargs=None):
            Count.n += 1
            return func(*args, **(kwargs or {}))

    def med(ts):
        ts = sorted(ts)
        return dict(p50=round(ts[len(ts) // 2], 5), p10=round(ts[len(ts) // 10], 5), p90=round(ts[(9 * len(ts)) // 10], 5))

    def measure(pair):
        for _ in range(args.warmup):
            pair()
        torch.cuda.synchronize()
        host, evs = [], []
        for _ in range(args.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0 = time.perf_counter()
            e0.record()
            pair()
            e1.record()
            torch.cuda.synchronize()
            host.append((time.perf_counter() - t0) * 1e3)
            evs.append(e0.elapsed_time(e1))
        Count.n, _lib.CALL_COUNT = 0, 0
        with Count():
            pair()
        calls, _lib.CALL_COUNT = _lib.CALL_COUNT, None
        torch.cuda.synchronize()
        return dict(host_ms=med(host), gpu_events_ms=med(evs), c_abi_calls=calls, aten_ops=Count.n)

    out = dict(tool="s3im_bench", rays=N, patch_hw=list(hw), repeat_time=R, kernel_size=k, stride=s, repeats=args.repeats,
               warmup=args.warmup, device=torch.cuda.get_device_name(0))
    pairs, vals = {}, {}
    for tag, fn in (("hip", losses.s3im_loss), ("torch", torch_s3im)):
        def pair(fn=fn):
            p = pred0.detach().requires_grad_(True)
            v = fn(p, gt, index, hw, k, s)
            v.backward()
            return v, p.grad
        pairs[tag] = measure(pair)
        vals[tag] = pair()
    torch.cuda.synchronize()
    out["fwd_bwd_pair"] = pairs
    out["fwd_bwd_pair_ratio_torch_over_hip"] = dict(
        host=round(pairs["torch"]["host_ms"]["p50"] / pairs["hip"]["host_ms"]["p50"], 3),
        gpu_events=round(pairs["torch"]["gpu_events_ms"]["p50"] / pairs["hip"]["gpu_events_ms"]["p50"], 3))
    out["fwd_bwd_pair_agreement"] = dict(value=float((vals["hip"][0] - vals["torch"][0]).abs()),
                                         grad_rel=float((vals["hip"][1] - vals["torch"][1]).abs().max() / vals["torch"][1].abs().max()))
    if not args.no_step:
        import bench
        trs = {}
        for mode in ("fused", "autograd", "s3im"):
            torch.manual_seed(0)
            tr = bench.build_trainer(dev, 0, 1, fused_step=(mode == "fused"))
            if mode == "s3im":
                tr.use_s3im(args.w, dict(patch_height=hw[0], patch_width=hw[1], repeat_time=R, kernel_size=k, stride=s))
            trs[mode] = [tr, 0]
        blocks, host = {m: [] for m in trs}, {m: [] for m in trs}
        calls = {}
        for m, st in trs.items():           # warm-up: occupancy refreshes, allocator, the first prefetch
            for _ in range(max(args.warmup, 30)):
                st[0].train_step(st[1])
                st[1] += 1
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for m, st in trs.items():
                for _ in range(args.blocks):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.block):
                        st[0].train_step(st[1])
                        st[1] += 1
                    t1 = time.perf_counter()
                    torch.cuda.synchronize()
                    blocks[m].append((time.perf_counter() - t0) * 1e3 / args.block)
                    host[m].append((t1 - t0) * 1e3 / args.block)
        for m, st in trs.items():
            _lib.CALL_COUNT = 0
            st[0].train_step(st[1])
            st[1] += 1
            calls[m], _lib.CALL_COUNT = _lib.CALL_COUNT, None
        torch.cuda.synchronize()
        out["rays_per_step"] = trs["fused"][0].num_rays
        out["train_step_ms"] = {m: med(b) for m, b in blocks.items()}
        out["train_step_host_ms"] = {m: med(b) for m, b in host.items()}
        out["train_step_c_abi_calls"] = calls
        p50 = {m: out["train_step_ms"][m]["p50"] for m in trs}
        out["train_step_ratio_s3im_over_autograd"] = round(p50["s3im"] / p50["autograd"], 4)
        out["train_step_ratio_s3im_over_fused"] = round(p50["s3im"] / p50["fused"], 4)
        out["train_step_cost_of_the_term_ms"] = round(p50["s3im"] - p50["autograd"], 5)
        out["rgb_s3im_after"] = dict(steps=trs["s3im"][1], value=float(trs["s3im"][0].loss_parts["rgb_s3im"]))
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
