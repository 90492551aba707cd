"""Average duration of the CLIP attention kernels (forward, backward) at B images of T tokens (development aid):
    python scripts/attn_time.py [--tokens T] [B ...]
Without arguments: T = 50 (ViT-B/32) at B = 2, 512 and T = 197 (ViT-B/16, the tiled kernels) at B = 1, 2, 64.  Next to every line,
torch.nn.functional.scaled_dot_product_attention on the same device and the same values in bf16 ([B, 12, T, 64] views of the same qkv;
forward, and backward of all three inputs) and the ratio ours / SDPA.
A/B against another commit: AVC_LIB_NAME=libavc_ref.so (scripts/build_ref.sh).  The A/B against the fp32 VALU kernels of round 3 is
profiles/r03_ab_kernels.txt."""
import os, sys
import torch
import torch.nn.functional as F
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from avatarclip_amd import clip_vit as V

args = sys.argv[1:]
tokens = None
if "--tokens" in args:
    i = args.index("--tokens")
    tokens = int(args[i + 1])
    del args[i:i + 2]
sizes = [int(a) for a in args]
if tokens is None:
    cases = [(50, B) for B in sizes or [2, 512]] + ([] if sizes else [(197, B) for B in (1, 2, 64)])
else:
    cases = [(tokens, B) for B in sizes or [1, 2, 64]]


def timed(fwd, bwd, n):
    """fwd() -> output, bwd(output): n forwards then n backwards, second of two rounds -> (forward us, backward us)"""
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
    for rep in range(2):
        outs = []
        ev[0].record()
        for _ in range(n):
            outs.append(fwd())
        ev[1].record()
        for o in outs:
            bwd(o)
        ev[2].record()
        torch.cuda.synchronize()
    return 1e3 * ev[0].elapsed_time(ev[1]) / n, 1e3 * ev[1].elapsed_time(ev[2]) / n


for T, B in cases:
    n = 200 if B * T <= 30000 else 50
    qkv = torch.randn(B, T, 2304, device="cuda", requires_grad=True)
    do = torch.randn(B, T, 768, device="cuda")
    f_us, b_us = timed(lambda: V.AttentionFn.apply(qkv), lambda o: o.backward(do), n)
    qkv.grad = None
    q, k, v = (t.reshape(B, T, 12, 64).permute(0, 2, 1, 3).bfloat16().detach().requires_grad_(True) for t in qkv.detach().split(768, dim=-1))
    dob = do.reshape(B, T, 12, 64).permute(0, 2, 1, 3).bfloat16()
    sf_us, sb_us = timed(lambda: F.scaled_dot_product_attention(q, k, v), lambda o: o.backward(dob), n)
    print("T=%d B=%d  %s  forward %.1f us  backward (incl. autograd) %.1f us   SDPA bf16 forward %.1f us backward %.1f us   ours / SDPA %.2f / %.2f"
          % (T, B, os.environ.get("AVC_LIB_NAME", "libavc.so"), f_us, b_us, sf_us, sb_us, f_us / sf_us, b_us / sb_us))
