"""Whole-iteration parity: Runner.train_clip_iteration (main.py:345-566) on the HIP path vs ONE INDEPENDENT iteration built
from the CPU oracle only (oracle/iteration_oracle.py: oracle render + cast_light + scatter + losses + clip_preprocess + ViT
oracle + Adam; it imports nothing of the product's Runner / renderer / engine), with identical weights, cameras, jitter,
backgrounds, lights and ambience.  Covers rows a1-a18 of SURVEY section 8 in one pass.

  * small nets (confs/examples_small), 32 x 32 rays x 32 spp, 2 iterations (the second one after an Adam step);
  * FULL-SIZE nets (confs/examples), 64 x 64 rays x 64 spp = BASELINE config 1's geometry, 1 iteration (CPU leg ~10 s);
  * silhouette-ray mode with a gaussian background (ragged ray set + scatter), small nets.

Tolerances (f16 forward / bf16 gradient operands against the fp32 oracle; measured values in DESIGN.md section 2):
per-iteration loss within 2e-3 (the loss is O(1)); per-tensor gradient: relative L2 <= 2e-2 against max(own norm, 1e-4 of
the whole gradient) and cosine >= 0.999; the scalar d loss / d (sdf bias) is a sum with heavy cancellation and has its own
5 % bound; rendered CLIP image max |diff| <= 5e-3.
"""
import os

import numpy as np
import pytest
import torch

gpu = pytest.mark.gpu


def _make_runner(device, res, spp, small=True, **over):
    import bench
    from avatarclip_amd.runner import Runner
    conf = bench.make_conf(res, spp, small=small)
    conf.put("train.use_bg_aug", False)
    conf.put("train.warm_up_end", 0)
    for k, v in over.items():
        conf.put(k, v)
    torch.manual_seed(0)
    r = Runner(None, mode="train_clip", conf=conf, device=device)
    return r


def _oracle_conf(r, res):
    return dict(H=res, W=res, focal=r.dataset.focal, n_samples=r.renderer.n_samples, n_importance=r.renderer.n_importance,
                up_sample_steps=r.renderer.up_sample_steps, full_frame_resolution_level=r.full_frame_resolution_level,
                mask_weight=r.mask_weight, igr_weight=r.igr_weight, clip_weight=r.clip_weight, add_no_texture=r.add_no_texture,
                texture_cast_light=r.texture_cast_light, use_face_prompt=r.use_face_prompt, use_back_prompt=r.use_back_prompt,
                use_silhouettes=r.use_silhouettes, cos_anneal_ratio=r.get_cos_anneal_ratio(), extra_color=True)


def _check_grads(names, grads_a, grads_b, sdf_last_bias, rel_tol, cos_tol, bias_tol):
    worst = 0.0
    seen_sdf = False
    gnorm = torch.cat([g.reshape(-1) for g in grads_b]).double().norm().item()
    for n, ga, gb in zip(names, grads_a, grads_b):
        if gb.abs().max() < 1e-7:
            continue
        if n == sdf_last_bias and not seen_sdf:
            # d loss / d (sdf bias) = sum over all points of d loss / d sdf: the eikonal and the alpha terms pull both ways and
            # cancel to ~1e-3 of sum |d_sdf|, so 1e-3-level forward differences (f16 operands) move this ONE scalar by a few
            # percent.  It is checked on its own with a wider bound; the other entries go through the common check.
            seen_sdf = True
            assert abs(ga.reshape(-1)[0] - gb.reshape(-1)[0]) < bias_tol * abs(gb.reshape(-1)[0]) + 1e-4, \
                ("sdf bias[0]", ga.reshape(-1)[0].item(), gb.reshape(-1)[0].item())
            ga, gb = ga.reshape(-1)[1:], gb.reshape(-1)[1:]
        # tensors whose gradient is below 1e-4 of the whole gradient (the 3-entry weight_g of the extra colour head, fed only
        # by the CLIP term) are compared against that floor, not against their own norm
        rel = ((ga - gb).double().norm() / (gb.double().norm() + 1e-4 * gnorm)).item()
        cos = torch.nn.functional.cosine_similarity(ga.reshape(1, -1).double(), gb.reshape(1, -1).double()).item()
        if gb.double().norm() < 1e-3 * gnorm:
            cos = 1.0
        worst = max(worst, rel)
        if os.environ.get("AVC_TEST_VERBOSE"):
            print("    %-24s rel %.3e cos %.6f |ref| %.3e" % (n, rel, cos, gb.double().norm().item()))
        assert rel < rel_tol and cos > cos_tol, (n, rel, cos)
    return worst


def _run_parity(res, spp, iters, small, silhouettes=False, rel_tol=2e-2, cos_tol=0.999, bias_tol=0.05, loss_tol=2e-3, warm_up_end=0,
                start_step=0):
    from oracle import iteration_oracle as IT
    from oracle import neus_oracle as O
    from avatarclip_amd.runner import clip_vit_random_state_dict, EllipsoidPrior
    clip_sd = clip_vit_random_state_dict(0)
    dev = torch.device("cuda")
    over = {}
    if silhouettes:
        over = {"train.use_silhouettes": True, "train.max_ray_num": 900, "dataset.H": 256, "dataset.W": 256}
    if warm_up_end:
        over["train.warm_up_end"] = warm_up_end
    a = _make_runner(dev, res, spp, small, **over)
    a.iter_step = start_step
    assert a.warm_up_end == warm_up_end
    a.init_clip(clip_state_dict=clip_sd)
    prior = EllipsoidPrior(device="cpu")
    cams = [(np.array([0.35, 0.25, 1.45], np.float32), np.array([0.02, -0.03, 0.01], np.float32), 0.3, 1.2, 1),
            (np.array([-1.1, 0.1, -0.9], np.float32), np.array([0.0, 0.05, 0.0], np.float32), 2.8, 4.0, 0)][:iters]
    priors = [prior(c[0], c[1]) for c in cams]
    step = {"i": 0}
    a.init_smpl(prior_renderer=lambda eye, at: priors[step["i"]].to(dev))
    a.update_learning_rate()
    # ---------------- the oracle leg: plain tensors + Adam, no product code
    sd_s = {n: p.detach().cpu().clone().requires_grad_() for n, p in a.sdf_network.named_parameters()}
    sd_c = {n: p.detach().cpu().clone().requires_grad_() for n, p in a.color_network.named_parameters()}
    var = a.deviation_network.variance.detach().cpu().clone().requires_grad_()
    st = IT.OracleState(sd_s, sd_c, var, lr0=a.learning_rate, alpha=a.learning_rate_alpha, warm_up_end=a.warm_up_end,
                        end_iter=a.end_iter, iter_step=start_step)
    assert abs(st.opt.param_groups[0]["lr"] - a.optimizer.param_groups[0]["lr"]) < 1e-12
    texts = dict(prompt=a.encoded_text.cpu(), face_prompt=a.encoded_face_text.cpu(), back_prompt=a.encoded_back_text.cpu())
    oconf = _oracle_conf(a, a.dataset.H)
    names = [n for net in (a.sdf_network, a.deviation_network, a.color_network) for n, _ in net.named_parameters()]
    sdf_last_bias = [n for n, _ in a.sdf_network.named_parameters() if n.endswith(".bias")][-1]
    a_render = a.renderer.render
    jit = {}
    a.renderer.render = lambda *args, **kw: a_render(*args, jitter=jit["t"].to(dev), **kw)
    bgs = {}
    if silhouettes:   # the gaussian background (choice 1) is an input of both legs
        a_draw = a.draw_background

        def draw(view, choice_i=None):
            g = torch.Generator().manual_seed(77 + step["i"])
            bg = torch.clamp(torch.normal(torch.zeros(view.H, view.W, 1) + 0.5, torch.zeros(view.H, view.W, 1) + 0.2, generator=g), 0, 1).reshape(-1, 1)
            bgs["bg"] = bg
            bgd = bg.to(dev)
            return 1, bgd, bgd.reshape(view.H, view.W, 1)[view.dilated_mask].reshape(-1, 1)
        a.draw_background = draw
    worst = 0.0
    for i in range(iters):
        step["i"] = i
        eye, at, theta, phi, is_front = cams[i]
        view = None
        if silhouettes:   # ragged ray set: take the product's (pinned by tests/test_oracle_golden.py against the reference)
            view = a.make_view(i, cams[i])
            R = view.rays_o.shape[0]
        else:
            R = int(a.dataset.W // a.full_frame_resolution_level) ** 2
        jit["t"] = torch.rand(R, 1, generator=torch.Generator().manual_seed(100 + i))
        np.random.seed(4321 + i)
        w_before = [p.detach().cpu().clone() for p in a.params_to_train]
        wo_before = [p.detach().clone() for p in st.params()]
        for pa, pb in zip(w_before, wo_before):       # the two legs start every iteration from (nearly) the same weights
            assert (pa - pb).abs().max() <= 2.5 * a.learning_rate
        lr_used = a.optimizer.param_groups[0]["lr"]
        if warm_up_end:      # the linear ramp of main.py:577-580, both legs
            assert abs(lr_used - a.learning_rate * (start_step + i) / warm_up_end) < 1e-12 and start_step + i < warm_up_end
            assert abs(st.opt.param_groups[0]["lr"] - lr_used) < 1e-12
        la = a.train_clip_iteration(i, camera=cams[i])
        grads_a = [p.grad.detach().cpu().clone() for p in a.params_to_train]
        a.update_learning_rate()
        rs = np.random.RandomState(4321 + i)          # the product drew: light angles (2), ambience (1)  (main.py:433,440)
        light = O.sphere_coord(theta + rs.uniform(-np.pi / 4, np.pi / 4), phi + rs.uniform(-np.pi / 4, np.pi / 4))
        amb = float(rs.uniform(0, 0.2))
        dr = IT.Draws(eye=eye, at=at, theta=theta, phi=phi, is_front=is_front, prior_rgb=priors[i], jitter=jit["t"],
                      choice_i=1 if silhouettes else 3, background_rgb=bgs.get("bg"), light_dir=light, ambience=amb)
        if silhouettes:
            dr.dilated_mask, dr.rays_o, dr.rays_d, dr.W = view.dilated_mask.cpu(), view.rays_o.cpu(), view.rays_d.cpu(), view.W
        ob = IT.train_clip_iteration(st, oconf, dr, clip_sd, texts, i)
        print("iter %d  loss hip %.6f oracle %.6f   cosine %.5f / %.5f" % (i, la.item(), ob["loss"].item(),
                                                                            a.last_stats["cosine"].item(), ob["cosine"].item()))
        assert abs(la.item() - ob["loss"].item()) < loss_tol * max(1.0, abs(ob["loss"].item()))
        assert abs(a.last_stats["cosine"].item() - ob["cosine"].item()) < 1e-3
        w = _check_grads(names, grads_a, ob["grads"], sdf_last_bias, rel_tol, cos_tol, bias_tol)
        worst = max(worst, w)
        # after the Adam step: both legs must have MOVED every significant weight the same way by (nearly) the same amount.
        # Adam's update is ~lr * sign(g) on the first step, so a bound of a few lr on |w_hip - w_oracle| cannot fail (a sign-flipped
        # gradient gives 2 lr); instead, on the entries whose gradient is above 1e-2 of the tensor's largest one (about half of all
        # entries): the two displacements share their sign and agree to 0.2 lr, each on >= 99 % of those entries.  (With the cut
        # at 1e-3 an unbiased per-entry error of 0.7 % of the tensor's RMS -- what bf16 operands give -- already flips 2 % of the
        # entries next to the cut in the second iteration; at 1e-2 errors up to 1.5 % pass and a flipped sign scores 0 %.)
        agree_min, close_min = 1.0, 1.0
        for n, w0, wo0, pa, pb, gb in zip(names, w_before, wo_before, a.params_to_train, st.params(), ob["grads"]):
            sel = gb.abs() > 1e-2 * gb.abs().max()
            if gb.abs().max() < 1e-7 or sel.sum() == 0:
                continue
            da, db = (pa.detach().cpu() - w0)[sel], (pb.detach() - wo0)[sel]
            agree = (torch.sign(da) == torch.sign(db)).float().mean().item()
            close = ((da - db).abs() <= 0.2 * lr_used + 1e-9).float().mean().item()
            agree_min, close_min = min(agree_min, agree), min(close_min, close)
            assert db.abs().max() > 0.5 * lr_used, (n, "the oracle leg did not step")
            assert agree >= 0.99 and close >= 0.99, (n, agree, close, int(sel.sum()))
        print("iter %d  Adam displacement: sign agreement >= %.4f, |w_hip - w_oracle| <= 0.2 lr on >= %.4f of the significant entries"
              % (i, agree_min, close_min))
    print("worst per-tensor relative gradient error", worst)
    return worst


@gpu
def test_train_clip_iteration_matches_independent_oracle_iteration_small_nets():
    _run_parity(res=32, spp=32, iters=2, small=True)


@gpu
def test_train_clip_iteration_matches_independent_oracle_iteration_full_size_nets():
    """BASELINE config 1 geometry (64 x 64 rays, S = I = 32) with the 256-wide networks of confs/examples."""
    _run_parity(res=64, spp=64, iters=1, small=False)


@gpu
def test_train_clip_iteration_at_128_samples_per_ray_matches_independent_oracle_iteration():
    """BASELINE config 3's sampling regime: 64 coarse + 64 importance samples per ray in four steps of 16 (the 32-lane up-sampling
    kernel, S = 128 rows through the training forward, the compositing scans and both backward kernels), full-size nets."""
    _run_parity(res=32, spp=128, iters=1, small=False)


@gpu
def test_train_clip_iterations_inside_the_learning_rate_warm_up():
    """main.py:571-586's linear warm-up branch (every other parity leg runs with warm_up_end = 0): two iterations at steps 3 and 4 of a
    10-step ramp; the Adam displacements are compared against the oracle's at the ramp's learning rates."""
    _run_parity(res=32, spp=32, iters=2, small=True, warm_up_end=10, start_step=3)


@gpu
def test_train_clip_iteration_silhouette_rays_matches_independent_oracle_iteration():
    _run_parity(res=256, spp=32, iters=1, small=True, silhouettes=True)


@gpu
@pytest.mark.parametrize("extra_color", [True, False])
def test_runner_train_neus_init_and_checkpoint_round_trip(tmp_path, extra_color):
    """Runner.train (main.py:180-256, BASELINE config 1) on a synthetic 4-image dataset in the reference's on-disk format
    (transforms_train.json + PNGs): the loss falls, the checkpoint has the reference's keys (main.py:622-629) and resumes."""
    import json
    from PIL import Image
    import bench
    from oracle import neus_oracle as O
    from avatarclip_amd.runner import Runner
    res = 32
    data = tmp_path / "data"
    (data / "img").mkdir(parents=True)
    frames = []
    yy, xx = np.mgrid[0:res, 0:res]
    for k in range(4):
        ang = 2 * np.pi * k / 4
        eye = np.array([1.5 * np.sin(ang), 0.2, 1.5 * np.cos(ang)])
        pose = O.lookat(eye, np.zeros(3), np.array([0., 1, 0]))
        disk = ((xx - res / 2 + 0.5) ** 2 + (yy - res / 2 + 0.5) ** 2) < (0.3 * res) ** 2     # a sphere seen from anywhere
        img = np.zeros((res, res, 3), np.uint8)
        img[disk] = (200, 150 + 20 * k, 100)
        Image.fromarray(img).save(str(data / "img" / ("%04d.png" % k)))
        frames.append({"file_path": "img/%04d" % k, "transform_matrix": np.asarray(pose).tolist()})
    with open(data / "transforms_train.json", "w") as fp:
        json.dump({"camera_angle_x": float(np.pi / 3), "frames": frames}, fp)
    conf = bench.make_conf(res, 32, small=True)
    conf.put("general.base_exp_dir", str(tmp_path / "exp"))
    conf.put("dataset.data_dir", str(data))
    conf.put("train.end_iter", 30)
    conf.put("train.batch_size", 256)
    conf.put("train.warm_up_end", 0)
    conf.put("train.save_freq", 30)
    # confs/base_models/*.conf (the NeuS-init stage) have no extra colour head; confs/examples/*.conf do
    conf.put("model.rendering_network.extra_color", extra_color)
    conf.put("model.neus_renderer.extra_color", extra_color)
    torch.manual_seed(0)
    np.random.seed(0)
    dev = torch.device("cuda")
    runner = Runner(None, mode="train", conf=conf, device=dev)
    assert runner.dataset.n_images == 4
    assert ("extra_lin.weight_v" in runner.color_network.state_dict()) == extra_color
    first = runner.train_iteration(runner.dataset.gen_random_rays_at(0, 256)).item()
    runner.train()
    last = runner.train_iteration(runner.dataset.gen_random_rays_at(0, 256)).item()
    print("NeuS-init loss", first, "->", last)
    assert np.isfinite(first) and np.isfinite(last) and last < first
    ck = tmp_path / "exp" / "checkpoints" / "ckpt_000030.pth"
    assert ck.exists()
    blob = torch.load(str(ck), map_location="cpu", weights_only=False)
    assert set(blob.keys()) == {"sdf_network_fine", "variance_network_fine", "color_network_fine", "optimizer", "iter_step"}
    assert any(k.endswith("weight_g") for k in blob["sdf_network_fine"]) and "variance" in blob["variance_network_fine"]
    r2 = Runner(None, mode="train", conf=conf, device=dev)
    r2.load_checkpoint("ckpt_000030.pth")
    assert r2.iter_step == 30
    sd_now = {k: v.clone() for k, v in blob["sdf_network_fine"].items()}
    for k, v in r2.sdf_network.state_dict().items():
        assert torch.equal(v.cpu(), sd_now[k].cpu())
    # --is_continue picks the newest checkpoint not past end_iter (main.py:160-170); train_clip's --pretrain path loads the
    # three networks of a NeuS-init checkpoint into the CLIP stage (main.py:611-620, strict=False for the colour head)
    r3 = Runner(None, mode="train", conf=conf, device=dev, is_continue=True)
    assert r3.iter_step == 30
    conf.put("train.pretrain", str(ck))
    r4 = Runner(None, mode="train_clip", conf=conf, device=dev)
    for k, v in r4.sdf_network.state_dict().items():
        assert torch.equal(v.cpu(), sd_now[k].cpu())
    # validate_image (main.py:741-820): one view rendered in ray chunks
    img = r4.validate_image(idx=0, resolution_level=2)
    assert img.shape == (16, 16, 3) and torch.isfinite(img).all() and img.min() >= 0 and img.max() <= 1


@gpu
def test_gaussian_background_draw_equals_torch_normal_of_tensors_on_the_device():
    """draw_background's choice 1 (main.py:393-394: torch.normal(zeros + 0.5, zeros + 0.2)) is written as randn * 0.2 + 0.5 -- the same
    draws without the host-side validation of the std tensor (a stream synchronisation per iteration)"""
    dev = torch.device("cuda")
    torch.manual_seed(7)
    a = torch.normal(torch.zeros([96, 96, 1], device=dev) + 0.5, torch.zeros([96, 96, 1], device=dev) + 0.2)
    torch.manual_seed(7)
    b = torch.randn([96, 96, 1], device=dev) * 0.2 + 0.5
    assert torch.equal(a, b)


@gpu
def test_train_clip_iteration_with_silhouette_rays_and_background_augmentation():
    """the reference's default sampling mode (use_silhouettes = True, main.py:360-375): a ragged, per-iteration ray set inside the
    dilated SMPL silhouette, scattered back into the image for CLIP, with every background augmentation (main.py:387-415)"""
    import bench
    from avatarclip_amd.runner import Runner
    conf = bench.make_conf(256, 32, small=True)
    conf.put("train.use_silhouettes", True)
    conf.put("train.max_ray_num", 3000)
    conf.put("train.warm_up_end", 0)
    torch.manual_seed(0)
    np.random.seed(3)
    r = Runner(None, mode="train_clip", conf=conf, device=torch.device("cuda"))
    r.init_clip()
    r.init_smpl()
    r.update_learning_rate()
    seen = set()
    for i in range(8):
        loss = r.train_clip_iteration(i)
        assert torch.isfinite(loss), i
        seen.add(int(r.last_stats["rays"]))
        r.update_learning_rate()
    assert len(seen) > 1 and max(seen) <= 3000 * 1.3      # ragged ray counts that respect the budget
    assert all(torch.isfinite(p).all() for p in r.params_to_train)


@gpu
def test_side_stream_view_keeps_the_draw_order_and_the_losses():
    """Runner.make_view_on_side_stream (silhouette mode: the iteration's view enqueued on a second HIP stream, the shipped default): same
    cameras, same ray sets, same background choices and the same losses as the run that builds every view on the main stream
    (Runner.overlap_view = False) -- the numpy draw order of main.py:348-440 is untouched.  (Full-frame mode uses no side stream.)"""
    import bench
    from avatarclip_amd.runner import Runner

    def run(overlap):
        conf = bench.make_conf(256, 32, small=True)
        conf.put("train.use_silhouettes", True)
        conf.put("train.max_ray_num", 3000)
        conf.put("train.warm_up_end", 0)
        torch.manual_seed(0)
        np.random.seed(3)
        r = Runner(None, mode="train_clip", conf=conf, device=torch.device("cuda"))
        if not overlap:
            r.overlap_view = False
        r.init_clip()
        r.init_smpl()
        r.update_learning_rate()
        rec = []
        for i in range(6):
            loss = r.train_clip_iteration(i)
            rec.append((np.asarray(r.last_view.eye).copy(), int(r.last_stats["rays"]), float(loss)))
            r.update_learning_rate()
        assert (r._side_stream is not None) == overlap
        return rec
    a, b = run(True), run(False)
    for (e1, n1, l1), (e2, n2, l2) in zip(a, b):
        assert np.array_equal(e1, e2) and n1 == n2
    assert abs(a[0][2] - b[0][2]) < 1e-5
    assert all(abs(x[2] - y[2]) < 5e-2 * max(1.0, abs(y[2])) for x, y in zip(a, b))     # (later iterations: fp32 summation order of the gradient scatter)


@gpu
@pytest.mark.parametrize("flags", [dict(add_no_texture=False, texture_cast_light=False, use_face_prompt=False, use_back_prompt=False),
                                   dict(add_no_texture=False, texture_cast_light=True, use_face_prompt=True, use_back_prompt=False),
                                   dict(add_no_texture=True, texture_cast_light=False, use_face_prompt=False, use_back_prompt=True)])
def test_train_clip_ablation_switches(flags):
    """the switch combinations of confs/ablation/*.conf (main.py:426-534): every branch of the shading / CLIP-loss glue runs"""
    import bench
    from avatarclip_amd.runner import Runner
    conf = bench.make_conf(64, 32, small=True)
    for k, v in flags.items():
        conf.put("train." + k, v)
    conf.put("train.use_bg_aug", False)
    torch.manual_seed(0)
    np.random.seed(5)
    r = Runner(None, mode="train_clip", conf=conf, device=torch.device("cuda"))
    r.init_clip()
    r.init_smpl()
    r.update_learning_rate()
    for i in range(5):          # i = 0 and 4 take the face-prompt camera when enabled (iter_i % 4 == 0)
        loss = r.train_clip_iteration(i)
        assert torch.isfinite(loss), (flags, i)
        r.update_learning_rate()
    assert all(torch.isfinite(p).all() for p in r.params_to_train)


@gpu
def test_cli_train_clip_from_a_conf_file(tmp_path):
    """`python -m avatarclip_amd.main --mode train_clip --conf X` (the reference's entry point, main.py:947-980) end to end:
    conf file on disk (reference syntax), the train_clip loop, report, checkpoint.  (`--case` is accepted and, as in the
    reference's Runner.__init__ (main.py:31-43), not substituted into the conf.)"""
    import subprocess
    import sys
    import bench
    conf = bench.make_conf(32, 32, small=True)
    # write the conf back out in the reference's HOCON style
    def dump(node, ind=0):
        out = []
        for k, v in node.items():
            if hasattr(v, "items"):
                out.append(" " * ind + "%s {" % k)
                out += dump(v, ind + 4)
                out.append(" " * ind + "}")
            else:
                out.append(" " * ind + "%s = %s" % (k, v))
        return out
    conf.put("general.base_exp_dir", str(tmp_path / "exp" / "smoke"))
    conf.put("train.end_iter", 3)
    conf.put("train.save_freq", 3)
    conf.put("train.report_freq", 1)
    conf.put("train.warm_up_end", 0)
    path = tmp_path / "case.conf"
    path.write_text("\n".join(dump(conf)) + "\n")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    p = subprocess.run([sys.executable, "-m", "avatarclip_amd.main", "--mode", "train_clip", "--conf", str(path), "--case", "smoke"],
                       cwd=root, capture_output=True, text=True, timeout=300)
    assert p.returncode == 0, p.stderr[-2000:]
    assert "loss" in p.stdout
    assert (tmp_path / "exp" / "smoke" / "checkpoints" / "ckpt_000003.pth").exists()


@gpu
def test_bench_dump_outputs_reproduce_run_to_run(tmp_path):
    """`bench.py --dump-outputs DIR` end to end: the result line names the files, they hold float32 / float64 arrays (<= 64 MB in all), and
    two runs with the same arguments write the same arrays (seeded inputs; an iteration is bit-reproducible)"""
    import json
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "AVC_DIST_BACKEND", "AVC_SINGLE_DEVICE"):
        env.pop(k, None)
    dumps = []
    for run in ("a", "b"):
        out_dir = str(tmp_path / run)
        cmd = [sys.executable, os.path.join(root, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1", "--res", "64", "--small",
               "--no-cpu-baseline", "--dump-outputs", out_dir]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600, cwd=root)
        assert r.returncode == 0, r.stderr[-3000:]
        line = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
        assert line["steps"] == 2 and line["ms_per_step"] > 0 and line["dumped_outputs"]["dir"] == out_dir
        files = line["dumped_outputs"]["files"]
        assert {"loss.npy", "color_loss.npy", "eikonal_loss.npy", "cosine.npy", "params.npy", "grads.npy"} <= set(files)
        assert sorted(files) == sorted(os.listdir(out_dir))
        arrays = {f: np.load(os.path.join(out_dir, f)) for f in files}
        assert all(a.dtype in (np.float32, np.float64) and np.isfinite(a).all() for a in arrays.values())
        assert sum(a.nbytes for a in arrays.values()) <= 64 << 20 and arrays["params.npy"].shape == arrays["grads.npy"].shape
        dumps.append(arrays)
    a, b = dumps
    assert sorted(a) == sorted(b)
    for f in a:
        assert np.array_equal(a[f], b[f]), (f, float(np.abs(a[f].astype(np.float64) - b[f]).max()))
