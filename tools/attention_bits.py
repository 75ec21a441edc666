"""Bitwise old-versus-new check of the head dim 128 attention bindings (``attention_d128_forward`` / ``_backward``):
``--save DIR`` on the tree before an edit of the kernels, ``--compare DIR`` on the tree after it.

The cases are tests/test_gpu_attention_d128.py's: B = 2, H = 2, S in {64, 128, 192, 1024} (one block with no
prefetch, the first prefetch, ring slot reuse, the widest hash index), both masks, p in {0, 0.1}, its seed.  The
inputs are drawn on the CPU, so a case does not depend on the device's generator, and no device seed base is
registered (ops.dropout_seed draws a new one per process): the masks are the host seed's alone.

    python tools/attention_bits.py --save DIR | --compare DIR     (exit status 1 at the first differing case)"""
import argparse
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

B, H, DH, SEED = 2, 2, 128, 12345
CASES = [(S, causal, p) for S in (64, 128, 192, 1024) for causal in (False, True) for p in (0.0, 0.1)]


def run(H_, S, causal, p):
    torch.manual_seed(41)
    qkv = (torch.randn(B, S, 3 * H * DH) * 1.5).bfloat16().cuda()
    dout = torch.randn(B, S, H * DH).bfloat16().cuda()
    out, lse = H_.attention_d128_forward(qkv, H, DH ** -0.5, SEED, p, causal)
    dqkv = H_.attention_d128_backward(qkv, out, lse, dout, H, DH ** -0.5, SEED, p, causal)
    return {"out": out.cpu(), "lse": lse.cpu(), "dqkv": dqkv.cpu()}


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    g = ap.add_mutually_exclusive_group(required=True)
    g.add_argument("--save", metavar="DIR")
    g.add_argument("--compare", metavar="DIR")
    args = ap.parse_args()
    from kungfu_amd._lib import hip

    if args.save:
        os.makedirs(args.save, exist_ok=True)
    for S, causal, p in CASES:
        name = "S%d_causal%d_p%g.pt" % (S, causal, p)
        got = run(hip(), S, causal, p)
        if args.save:
            torch.save(got, os.path.join(args.save, name))
            continue
        want = torch.load(os.path.join(args.compare, name))
        diff = [k for k in want if not torch.equal(got[k], want[k])]
        if diff:
            sys.exit("%s: %s differ from the saved tensors" % (name, ", ".join(diff)))
    print("%d cases %s" % (len(CASES), "saved" if args.save else "bitwise equal: out, lse, dqkv"))


if __name__ == "__main__":
    main()
