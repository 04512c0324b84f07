"""The measurements of DESIGN.md 4.17 (profiles/compile_micro.json), one mode per process:

    python scripts/compile_micro.py eager [--pkg DIR]     module-level SmoothnessLoss and MultiScale, forward + backward, us per call
    python scripts/compile_micro.py compiled --what unsup|flownet2c --how eager|aot_eager|reduce-overhead      ms per training step

``eager`` is the host-bound side: the wall clock over a synchronised window of calls.  ``--pkg`` names another checkout's
``flownet2-pytorch_amd`` (the parent commit's, with this build's extensions beside it), for an alternating comparison in one lease.
``compiled`` times the unsupervised recipe's step (8 x 3 x 384 x 512) or harness.FlowNet2C's training step with the MultiScale criterion:
device events around a synchronised window, after a warm-up that includes compilation; the backward stays outside the compiled function.
With ``--criterion inside`` and ``--how reduce-overhead`` the run raises: the criterion's binding caches its workspace per stream, and a
tensor allocated during CUDA-graph warm-up and kept alive outside the graph is refused by Inductor's graph trees.
Every mode prints one JSON line.
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def spread(xs):
    return {"median": round(statistics.median(xs), 4), "min": round(min(xs), 4), "max": round(max(xs), 4), "windows": len(xs)}


def eager(args):
    import torch
    import torch.nn.functional as F
    from losses_fused import MultiScale
    from networks.smoothness_package import SmoothnessLoss
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    flow = torch.randn(8, 2, 96, 128, generator=g).to(dev).requires_grad_(True)
    image = torch.rand(8, 3, 96, 128, generator=g).to(dev)
    smooth = SmoothnessLoss(order=2)
    target = (torch.randn(8, 2, 384, 512, generator=g) * 4).to(dev)
    outs = [F.avg_pool2d(target, 4 << i).mul(0.05).add(0.01).requires_grad_(True) for i in range(5)]
    crit = MultiScale()

    def smooth_fb():
        smooth(flow, image).backward()

    def multiscale_fb():
        crit(outs, target)[0].backward()

    res = {}
    for name, fn in (("smoothness_loss_us", smooth_fb), ("multiscale_us", multiscale_fb)):
        for _ in range(50):
            fn()
        times = []
        for _ in range(args.windows):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.calls):
                fn()
            torch.cuda.synchronize()
            times.append((time.perf_counter() - t0) / args.calls * 1e6)
        res[name] = spread(times)
    return res


def compiled(args):
    import torch
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(0)
    if args.what == "unsup":
        import compile_cases as CC
        import pipelines_ref as P
        layers = P.hip_layers()
        im1, im2 = (torch.rand(8, 3, 384, 512, generator=g).to(dev).requires_grad_(True) for _ in range(2))
        flow12 = (torch.randn(8, 2, 384, 512, generator=g) * 3).to(dev).requires_grad_(True)
        flow21 = (torch.randn(8, 2, 384, 512, generator=g) * 3).to(dev)
        leaves = [im1, im2, flow12]

        def forward():
            return CC.unsup_forward(layers, im1, im2, flow12, flow21)[0]
    else:
        from harness.flownet2c import FlowNet2C
        from losses_fused import MultiScale
        torch.manual_seed(0)
        model, crit = FlowNet2C().to(dev).train(), MultiScale()
        frames = (torch.rand(8, 3, 2, 384, 512, generator=g) * 255).to(dev)
        target = (torch.randn(8, 2, 384, 512, generator=g) * 4).to(dev)
        leaves = list(model.parameters())

        if args.criterion == "inside":
            def forward():
                return crit(model(frames), target)[0]
        else:       # the model alone is compiled; the criterion runs eagerly on its outputs
            net = model if args.how == "eager" else torch.compile(model, fullgraph=True, **(
                {"backend": "aot_eager"} if args.how == "aot_eager" else {"mode": "reduce-overhead"}))
            args.how_outer, args.how = args.how, "eager"

            def forward():
                return crit(net(frames), target)[0]

    fn = forward if args.how == "eager" else torch.compile(forward, fullgraph=True, **(
        {"backend": "aot_eager"} if args.how == "aot_eager" else {"mode": "reduce-overhead"}))

    def step():
        for t in leaves:
            t.grad = None
        if "reduce-overhead" in (args.how, getattr(args, "how_outer", "")):
            torch.compiler.cudagraph_mark_step_begin()
        fn().backward()

    t0 = time.perf_counter()
    for _ in range(args.warmup):
        step()
    torch.cuda.synchronize()
    warm = time.perf_counter() - t0
    times = []
    for _ in range(args.windows):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        start.record()
        for _ in range(args.steps):
            step()
        stop.record()
        torch.cuda.synchronize()
        times.append(start.elapsed_time(stop) / args.steps)
    args.how = getattr(args, "how_outer", args.how)
    res = {"what": args.what, "how": args.how, "criterion": args.criterion if args.what == "flownet2c" else None, "ms_per_step": spread(times), "warmup_s": round(warm, 1)}
    if args.how == "reduce-overhead":
        from torch._dynamo.utils import counters
        res["cudagraph_skips"] = int(counters["inductor"]["cudagraph_skips"])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["eager", "compiled"])
    ap.add_argument("--pkg", default=os.path.join(ROOT, "flownet2-pytorch_amd"))
    ap.add_argument("--what", choices=["unsup", "flownet2c"], default="unsup")
    ap.add_argument("--how", choices=["eager", "aot_eager", "reduce-overhead"], default="eager")
    ap.add_argument("--criterion", choices=["inside", "outside"], default="inside",
                    help="flownet2c: MultiScale inside the compiled function, or eager on the compiled model's outputs")
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--calls", type=int, default=300)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    res = eager(args) if args.mode == "eager" else compiled(args)
    res["mode"] = args.mode
    print(json.dumps(res))


if __name__ == "__main__":
    main()
