"""Time the fused layer-wise optimizer steps on flat spaces with ResNet-50's and BERT-base's slot lists.

    python tools/bench_layerwise.py [--iters 50] [--rounds 5] [--out profiles/layerwise_optimizers.md]
    python tools/bench_layerwise.py --slots        # slot lists only (no GPU needed)

In one process, per model: FusedLARS.step against FusedSGD.step, FusedLAMB.step against
FusedAdam.step, and each against the plain per-tensor LARS / LAMB (torch ops on the GPU).  No
training runs: the slot lists come from the models built on the meta device, the buffers hold random
numbers and the learning rate is tiny.  The variants alternate within every round and the median
round is reported; GB/s is the bytes each step has to move by its access pattern (LARS 28, SGD with
momentum 20, LAMB 40, Adam 28 bytes per flat element, no bf16 shadow) over that time.
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

BYTES = {"FusedSGD": 20, "FusedLARS": 28, "FusedAdam": 28, "FusedLAMB": 40}


def slot_list(name):
    """[(numel, ndim)] of the model's trainable parameters, in registration order."""
    from kungfu_amd.models import get_model

    try:
        with torch.device("meta"):
            m = get_model(name)
    except Exception:  # noqa: BLE001 -- a module that cannot be built on meta: build it on the CPU
        m = get_model(name)
    return [(p.numel(), p.ndim) for p in m.parameters() if p.requires_grad]


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters * 1e3  # us


def bench_model(name, iters, rounds):
    from kungfu_amd.optimizers import LAMB, LARS, FusedAdam, FusedLAMB, FusedLARS, FusedSGD
    from kungfu_amd.parallel.flat import FlatParamSpace

    slots = slot_list(name)
    dev = torch.device("cuda")
    g = torch.Generator(device=dev).manual_seed(0)

    def params():
        return [torch.nn.Parameter(torch.randn(n, device=dev, generator=g) * 0.02) for n, _ in slots]

    ps = params()
    sp = FlatParamSpace(ps)
    sp.flat_grad.copy_(torch.randn(sp.numel, device=dev, generator=g) * 1e-3)
    sp.flat_grad[_padding(sp)] = 0
    over = {p: dict(weight_decay=0.0, trust=False) for p, (_, nd) in zip(ps, slots) if nd == 1}
    lr = 1e-6
    fused = {
        "FusedSGD": FusedSGD(sp, lr=lr, momentum=0.9, weight_decay=1e-4),
        "FusedLARS": FusedLARS(sp, lr=lr, momentum=0.9, weight_decay=1e-4, overrides=over),
        "FusedAdam": FusedAdam(sp, lr=lr, weight_decay=0.01),
        "FusedLAMB": FusedLAMB(sp, lr=lr, weight_decay=0.01, overrides=over),
    }
    qs = params()
    for q in qs:
        q.grad = torch.randn(q.numel(), device=dev, generator=g) * 1e-3

    def groups():
        return [dict(params=[q for q, (_, nd) in zip(qs, slots) if nd > 1]),
                dict(params=[q for q, (_, nd) in zip(qs, slots) if nd == 1], weight_decay=0.0, trust=False)]

    plain = {"LARS": LARS(groups(), lr=lr, momentum=0.9, weight_decay=1e-4),
             "LAMB": LAMB(groups(), lr=lr, weight_decay=0.01)}
    steps = {k: o.step for k, o in {**fused, **plain}.items()}
    for f in steps.values():  # warm up: code objects, state buffers
        for _ in range(3):
            f()
    torch.cuda.synchronize()
    times = {k: [] for k in steps}
    for _ in range(rounds):
        for k, f in steps.items():  # alternate the variants inside every round
            times[k].append(timed(f, iters if k.startswith("Fused") else max(3, iters // 10)))
    res = {k: (statistics.median(v), min(v), max(v)) for k, v in times.items()}
    return dict(name=name, nseg=len(slots), numel=sp.numel, params=sum(n for n, _ in slots), res=res)


def _padding(sp):
    m = torch.ones(sp.numel, dtype=torch.bool, device=sp.device)
    for o, n in sp.offsets:
        m[o:o + n] = False
    return m


def report(rows, iters, rounds):
    out = ["| model | slots | flat elements | step | median us | min .. max us | bytes/elem | GB/s |",
           "|---|---|---|---|---|---|---|---|"]
    for r in rows:
        for k, (med, lo, hi) in r["res"].items():
            b = BYTES.get(k)
            gbs = "%.0f" % (b * r["numel"] / med / 1e3) if b else "-"
            out.append("| %s | %d | %d | %s | %.1f | %.1f .. %.1f | %s | %s |" %
                       (r["name"], r["nseg"], r["numel"], k, med, lo, hi, b or "-", gbs))
    out += ["", "| model | ratio | measured | by bytes |", "|---|---|---|---|"]
    for r in rows:
        t = {k: v[0] for k, v in r["res"].items()}
        out.append("| %s | FusedLARS / FusedSGD | %.2f | %.2f |" % (r["name"], t["FusedLARS"] / t["FusedSGD"], 28 / 20))
        out.append("| %s | FusedLAMB / FusedAdam | %.2f | %.2f |" % (r["name"], t["FusedLAMB"] / t["FusedAdam"], 40 / 28))
        out.append("| %s | plain LARS / FusedLARS | %.1f | - |" % (r["name"], t["LARS"] / t["FusedLARS"]))
        out.append("| %s | plain LAMB / FusedLAMB | %.1f | - |" % (r["name"], t["LAMB"] / t["FusedLAMB"]))
    out += ["", "%d steps per timed window for the fused steps (a tenth for the plain ones), %d rounds, "
            "device events around each window; %s." % (iters, rounds, torch.cuda.get_device_name(0))]
    return "\n".join(out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--models", default="resnet50,bert_base")
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the tables to this file")
    ap.add_argument("--slots", action="store_true", help="print the slot lists' sizes and exit")
    a = ap.parse_args()
    names = a.models.split(",")
    if a.slots:
        for n in names:
            s = slot_list(n)
            print("%s: %d slots, %d parameters, %d one-dimensional" % (n, len(s), sum(x for x, _ in s),
                                                                      sum(1 for _, d in s if d == 1)))
        return
    if not torch.cuda.is_available():
        sys.exit("bench_layerwise: needs a GPU (use --slots for the slot lists alone)")
    text = report([bench_model(n, a.iters, a.rounds) for n in names], a.iters, a.rounds)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
