"""Error-map importance sampling (neuralsim_amd/importance.py, kernels ``nsim_errmap_*``) at the size of the reference's object
configs: 100 images, ``error_map_hw`` (32, 64), 8192 rays per iteration.

1. One draw (``ImpSampler.sample_img_pixel``) plus one update (``ErrorMap.step_error_map``) with the HIP classes, beside the same
   two calls on the torch classes of ``nr3d_lib.models.importance`` on the device -- the path the HIP classes replace.  Per
   variant: the median of the host clock around a synchronised pair and of the HIP events around it, after ``--warmup`` pairs,
   and what one pair issues (C-ABI calls and ATen operator calls, counted once outside the timing).
2. The headline ``RenderTrainer`` step of bench.py (``build_trainer``) with ``pixel_sample_mode`` ``uniform`` and ``error_map``, and
   -- to tell the cost of the mechanism from the cost of the batches it draws -- ``update_only``: the map is updated every step but
   the batch stays uniform (``enable_after`` never reached).  Blocks of ``--block`` steps timed with one synchronisation at the end
   of a block (``host`` = the part of it the host spent issuing the steps), the modes alternated ``--rounds`` times in one process,
   medians over the blocks; with them the mean number of hit rays and with-grad samples per step of every mode.

Prints one JSON line.

    python tools/importance_bench.py [--rays 8192] [--repeats 50] [--warmup 10] [--out profiles/importance_bench.json]
"""
import argparse
import json
import sys
import time
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rays", type=int, default=8192)
    ap.add_argument("--images", type=int, default=100)
    ap.add_argument("--hw", type=int, nargs=2, default=[32, 64])
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
    from neuralsim_amd import _lib, importance as hip
    from nr3d_lib.models import importance as shim
    assert torch.cuda.is_available(), "importance_bench needs a HIP device"
    dev = torch.device("cuda", 0)
    V, hw, N = args.images, tuple(args.hw), args.rays
    gen = torch.Generator(device=dev).manual_seed(1)
    em0 = torch.rand([V, *hw], device=dev, generator=gen) ** 2 + 0.01
    val = torch.rand([N], device=dev, generator=gen)

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

    out = dict(tool="importance_bench", n_images=V, error_map_hw=list(hw), rays=N, repeats=args.repeats, warmup=args.warmup,
               device=torch.cuda.get_device_name(0))
    pairs = {}
    for tag, mod in (("hip", hip), ("torch", shim)):
        EM = mod.ErrorMap if tag == "hip" else mod.TorchErrorMap
        SM = mod.ImpSampler if tag == "hip" else mod.TorchImpSampler
        em = EM(V, error_map_hw=hw, device=dev)
        with torch.no_grad():
            em.error_map.copy_(em0)
        smp = SM({"error_map": (em, 1.0)}, frac_uniform=0.5)

        def pair(em=em, smp=smp):
            fidx, xy = smp.sample_img_pixel(N)
            em.step_error_map(fidx, xy, val)
        pairs[tag] = measure(pair)
    out["draw_plus_update"] = pairs
    out["draw_plus_update_ratio_torch_over_hip"] = dict(
        host=round(pairs["torch"]["host_ms"]["p50"] / pairs["hip"]["host_ms"]["p50"], 3),
        gpu_events=round(pairs["torch"]["gpu_events_ms"]["p50"] / pairs["hip"]["gpu_events_ms"]["p50"], 3))
    if not args.no_step:
        import bench
        trs = {}
        for mode in ("uniform", "update_only", "error_map"):
            torch.manual_seed(0)
            tr = bench.build_trainer(dev, 0, 1)
            if mode != "uniform":
                tr.use_error_map_sampling(dict(error_map_hw=hw, frac_uniform=0.5, min_pdf=0.01,
                                               enable_after=0 if mode == "error_map" else 10 ** 9))
            trs[mode] = [tr, 0]
        blocks, host, work = {m: [] for m in trs}, {m: [] for m in trs}, {m: [0, 0, 0] for m in trs}
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
                        work[m][0] += 1
                        work[m][1] += st[0].stats.get("R_hit", 0)
                        work[m][2] += st[0].stats.get("S_f", 0)
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
        out["train_step_ms"] = {m: med(b) for m, b in blocks.items()}
        out["train_step_host_ms"] = {m: med(b) for m, b in host.items()}
        out["train_step_work"] = {m: dict(R_hit=round(w[1] / w[0], 1), S_f=round(w[2] / w[0], 1)) for m, w in work.items()}
        out["train_step_c_abi_calls"] = calls
        out["train_step_ratio_update_only_over_uniform"] = round(out["train_step_ms"]["update_only"]["p50"] /
                                                                 out["train_step_ms"]["uniform"]["p50"], 4)
        out["train_step_ratio_error_map_over_uniform"] = round(out["train_step_ms"]["error_map"]["p50"] /
                                                               out["train_step_ms"]["uniform"]["p50"], 4)
        em = trs["error_map"][0].error_map
        out["error_map_after"] = dict(steps=trs["error_map"][1], min=float(em.error_map.min()), max=float(em.error_map.max()),
                                      n_steps_mean=float(em.n_steps.float().mean()))
    line = json.dumps(out)
    print(line)
    if args.out:
        Path(args.out).write_text(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
