"""bfloat16 against half and fp32, in one process: correlation forward / backward (FlowNetC's cost volume, C ABI, AUTO) at
8x256x48x64 and 8x256x56x128, ChannelNorm forward / backward at 8x3x384x512, and a FlowNet2C training step in fp32 against the
same step under bf16 autocast.  The dtypes alternate inside every repeat; each entry is the median (and min) of device-event times
over warmed repeats.  Also records the bf16 accuracy of the training step's flow against fp32 (relative RMS) and whether
v_mfma_f32_16x16x32_bf16 keeps a subnormal bf16 operand.

    python scripts/bf16_micro.py [--out profiles/bf16_micro.json] [--reps 30]     # prints the JSON; --out also writes it
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "flownet2-pytorch_amd")]

import torch  # noqa: E402

CORR = (20, 1, 20, 1, 2)


def timed(fns, reps, warm=5):
    """fns: {name: callable}; alternates them within each repeat; returns {name: {median_us, min_us}}."""
    for _ in range(warm):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            f()
            e.record()
            e.synchronize()
            ts[k].append(s.elapsed_time(e) * 1e3)
    out = {}
    for k, v in ts.items():
        v.sort()
        out[k] = {"median_us": round(v[len(v) // 2], 2), "min_us": round(v[0], 2)}
    return out


def corr_fns(shape, dev):
    import fn2_capi
    B, C, H, W = shape
    g = torch.Generator(device=dev).manual_seed(1)
    fns = {}
    for name, dt in (("bf16", torch.bfloat16), ("half", torch.float16), ("fp32", torch.float32)):
        a = torch.randn(B, C, H, W, device=dev, generator=g).to(dt)
        b = torch.randn(B, C, H, W, device=dev, generator=g).to(dt)
        out = torch.empty(B, 441, H, W, device=dev, dtype=dt)
        go = torch.randn(B, 441, H, W, device=dev, generator=g).to(dt)
        g1, g2 = torch.empty_like(a), torch.empty_like(b)
        fns["fwd_" + name] = (lambda a=a, b=b, out=out: fn2_capi.correlation_forward(a, b, *CORR, out=out))
        if W <= 64:   # the C ABI's bf16 / half backward kernels hold rows of <= 64 px (wider maps: the binding widens to fp32)
            fns["bwd_" + name] = (lambda a=a, b=b, go=go, g1=g1, g2=g2: fn2_capi.correlation_backward(a, b, go, *CORR, out=(g1, g2)))
        else:
            import correlation_cuda
            fns["bwd_" + name] = (lambda a=a, b=b, go=go: correlation_cuda.backward_alloc(a, b, go, *CORR, 1))
    return fns


def chnorm_fns(dev):
    import channelnorm_cuda
    fns = {}
    g = torch.Generator(device=dev).manual_seed(2)
    for name, dt in (("bf16", torch.bfloat16), ("half", torch.float16), ("fp32", torch.float32)):
        x = torch.randn(8, 3, 384, 512, device=dev, generator=g).to(dt)
        out = torch.empty(8, 1, 384, 512, device=dev, dtype=dt)
        go = torch.randn(8, 1, 384, 512, device=dev, generator=g).to(dt)
        gi = torch.empty_like(x)
        channelnorm_cuda.forward(x, out, 2)
        fns["fwd_" + name] = (lambda x=x, out=out: channelnorm_cuda.forward(x, out, 2))
        fns["bwd_" + name] = (lambda x=x, out=out, go=go, gi=gi: channelnorm_cuda.backward(x, out, go, gi, 2))
    return fns


def training_step(dev, reps, batch, height, width):
    from harness.flownet2c import FlowNet2C
    from harness.train import synthetic_batch
    from losses_fused import MultiScaleL1
    torch.manual_seed(1)
    model = FlowNet2C().to(dev).train()
    crit = MultiScaleL1()
    inputs, target = synthetic_batch(batch, height, width, dev)

    def step(dtype):
        model.zero_grad(set_to_none=True)
        if dtype is None:
            loss = crit(model(inputs), target)[0]
        else:
            with torch.autocast("cuda", dtype=dtype):
                loss = crit(model(inputs), target)[0]
        loss.backward()

    t = timed({"fp32": lambda: step(None), "bf16_autocast": lambda: step(torch.bfloat16)}, reps, warm=3)
    with torch.no_grad():
        f32 = model(inputs)[0].float()
        with torch.autocast("cuda", dtype=torch.bfloat16):
            f16 = model(inputs)[0].float()
    t["flow2_rel_rms_bf16_vs_fp32"] = float((f16 - f32).pow(2).mean().sqrt() / f32.pow(2).mean().sqrt())
    t["shape"] = [batch, 3, 2, height, width]
    return t


def subnormal_probe(dev):
    import fn2_capi
    a = torch.zeros(1, 128, 6, 8, dtype=torch.bfloat16)
    b = torch.zeros(1, 128, 6, 8, dtype=torch.bfloat16)
    a[:, 0] = 2.0 ** -130
    b[:, 0] = 2.0 ** 100
    v = fn2_capi.correlation_forward(a.to(dev), b.to(dev), *CORR)[0, 220].float().unique().tolist()
    return {"centre_values": v, "exact": 2.0 ** -30 / 128, "kept": v == [2.0 ** -30 / 128], "flushed": v == [0.0]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="also write the JSON result to this file")
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--step-reps", type=int, default=10)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "needs a GPU"
    dev = torch.device("cuda:0")
    res = {"device": torch.cuda.get_device_name(0), "reps": a.reps}
    for shape in ((8, 256, 48, 64), (8, 256, 56, 128)):
        res["corr_" + "x".join(map(str, shape))] = timed(corr_fns(shape, dev), a.reps)
        torch.cuda.empty_cache()
    res["chnorm_8x3x384x512"] = timed(chnorm_fns(dev), a.reps)
    res["subnormal_bf16_mfma"] = subnormal_probe(dev)
    res["flownet2c_train_step_2x384x512"] = training_step(dev, a.step_reps, 2, 384, 512)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
    print(json.dumps(res, indent=1))


if __name__ == "__main__":
    main()
