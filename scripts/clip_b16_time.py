"""The price of the finer CLIP tower (development aid): one Runner.train_clip_iteration at 224 x 224 rays x 64 samples per ray, full-size
nets, with seeded ViT-B/32 and ViT-B/16 stand-in weights on the same device, and the CLIP stretch on its own (encode_image of 2 images +
backward to the pixels, the graph-replayed per-iteration call).
    python scripts/clip_b16_time.py [patch ...]          (default: 32 16)
For the CLIP stretch from a kernel trace run ONE variant under the profiler: rocprofv3 --kernel-trace --stats -- python
scripts/clip_b16_time.py 16, and sum the vit_* kernels of the statistics table (AVC_B16_ITERS sets the number of timed iterations)."""
import os, sys, time
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from avatarclip_amd.runner import clip_vit_random_state_dict

dev = torch.device("cuda")
iters = int(os.environ.get("AVC_B16_ITERS", "20"))
for patch in [int(a) for a in sys.argv[1:]] or [32, 16]:
    torch.manual_seed(0)
    sd = clip_vit_random_state_dict(0, patch=patch)
    r = bench.build_runner(224, 64, False, dev)      # (as the benchmark builds it; then the tower is replaced)
    r.init_clip(clip_state_dict=sd)
    assert r.perceptor.patch == patch
    for i in range(5):
        r.train_clip_iteration(i); r.update_learning_rate()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for i in range(5, 5 + iters):
        r.train_clip_iteration(i); r.update_learning_rate()
    torch.cuda.synchronize()
    ms_iter = 1e3 * (time.perf_counter() - t0) / iters
    # the CLIP stretch alone: 2 images with a gradient, as Runner calls it with add_no_texture
    img = torch.randn(2, 3, 224, 224, device=dev)
    text = torch.randn(1, 512, device=dev)

    def clip_pass():
        x = img.clone().requires_grad_(True)
        e = r.perceptor.encode_image(x)
        (1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0)).backward()
    for _ in range(5):
        clip_pass()
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
    torch.cuda.synchronize()
    ev[0].record()
    for _ in range(iters):
        clip_pass()
    ev[1].record()
    torch.cuda.synchronize()
    print("ViT-B/%d (%d tokens)  train_clip iteration 224^2 x 64 spp: %.2f ms   CLIP forward + backward of 2 images (events): %.3f ms"
          % (patch, r.perceptor.tokens, ms_iter, ev[0].elapsed_time(ev[1]) / iters), flush=True)
    del r
