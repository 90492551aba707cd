"""What the packed pipeline buys a CLIP gradient call above 128 rows (development aid).  Seeded stand-in weights; every figure is the
median of AVC_PG_REPS (default 60, at least 50) repetitions timed one by one with events after a warm-up, with the spread (10th .. 90th
percentile, and the minimum) beside it:
  1. encode_image forward + backward of 1 and 2 ViT-B/16 images, replayed as HIP graphs (the per-iteration call of train_clip);
  2. the same of 5 ViT-B/32 images, eager launches (PoseOptimizer's call: 5 views of one pose);
  3. one Runner.train_clip_iteration at 224 x 224 rays x 64 samples per ray with ViT-B/16 stand-in weights.
    python scripts/clip_packed_grad_time.py [1] [2] [3]          (default: all three)
The script only uses what both sides of a comparison have: copy it into a checkout of the commit to compare against (its library built
there, or scripts/build_ref.sh + AVC_LIB_NAME) and run both in one job, alternating, on one device -- boxes differ by more than the
effect.  The first line names the route a 394-row gradient call takes in the checkout it runs in."""
import os, sys
import torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import bench
from avatarclip_amd import clip_vit as V
from avatarclip_amd.runner import clip_vit_random_state_dict

dev = torch.device("cuda")
reps = max(50, int(os.environ.get("AVC_PG_REPS", "60")))
which = [int(a) for a in sys.argv[1:]] or [1, 2, 3]


def timed(step, warm=8):
    """ms of every one of `reps` calls of step(i), events around each"""
    for i in range(warm):
        step(i)
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(reps)]
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(ev):
        a.record()
        step(warm + i)
        b.record()
    torch.cuda.synchronize()
    return sorted(a.elapsed_time(b) for a, b in ev)


def report(what, ms):
    q = lambda f: ms[min(len(ms) - 1, int(f * len(ms)))]
    print("%-78s median %7.3f ms   p10 %7.3f  p90 %7.3f  min %7.3f   (%d repetitions)" % (what, q(0.5), q(0.1), q(0.9), ms[0], len(ms)), flush=True)


def clip_pass(model, img, text):
    def step(_):
        x = img.clone().requires_grad_(True)
        e = model.encode_image(x)
        (1 - torch.cosine_similarity(e.mean(0), text.mean(0), dim=0)).backward()
    return step


torch.manual_seed(0)
text = torch.randn(1, 512, device=dev)
if 1 in which or 2 in which:
    m16 = V.ClipVision(clip_vit_random_state_dict(0, patch=16), dev)
    x = torch.randn(2, 3, 224, 224, device=dev).requires_grad_(True)
    before = set(m16._packed)
    m16._encode_image_eager(x).sum().backward()
    print("a 394-row gradient call runs %s" % ("the packed pipeline (BlocksFn)" if set(m16._packed) - before else "one autograd node per kernel"),
          flush=True)
if 1 in which:
    for B in (1, 2):
        img = torch.randn(B, 3, 224, 224, device=dev)
        ms = timed(clip_pass(m16, img, text))
        assert m16._graphed.get(B) not in (None, False)
        report("ViT-B/16 encode_image forward + backward, %d image%s (%d rows), HIP graphs:" % (B, "s" * (B > 1), 197 * B), ms)
if 2 in which:
    m32 = V.ClipVisionB32(clip_vit_random_state_dict(0), dev)
    img = torch.randn(5, 3, 224, 224, device=dev)
    report("ViT-B/32 encode_image forward + backward, 5 images (250 rows), eager launches:", timed(clip_pass(m32, img, text)))
if 3 in which:
    r = bench.build_runner(224, 64, False, dev)      # (as the benchmark builds it; then the tower is replaced)
    r.init_clip(clip_state_dict=clip_vit_random_state_dict(0, patch=16))
    assert r.perceptor.patch == 16

    def it(i):
        r.train_clip_iteration(i)
        r.update_learning_rate()
    report("train_clip iteration, 224^2 rays x 64 spp, ViT-B/16 stand-in weights:", timed(it, warm=6))
